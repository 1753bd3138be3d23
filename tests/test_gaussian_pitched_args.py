"""blur_gaussian_*_pitched_batch_dev and blur_gaussian_*_sigmas_pitched_batch_dev: argument validation that needs no device (the
checks run before the context is touched, so ctx may be NULL), the bindings, and the stride analysis of the Python wrapper
(api._gauss_strided_layout) on CPU tensors."""
import ctypes as C
import os
import re

import pytest

INVALID, UNSUPPORTED = 1, 2
TYPES = {"u8": 1, "u16": 2, "f32": 4, "f16": 2, "bf16": 2}          # entry name -> bytes per sample


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
ROWS, COLS = 40, 90          # sigma 2 fits (pad <= rows - 1), sigma 30 does not


def call(tname, per_channel, src_pitch, src_frame, dst_pitch, dst_frame, nframes=1, rows=ROWS, cols=COLS, ch=3, sigma=2.0, src=P, dst=P):
    o = opts()
    if per_channel:
        sg = (C.c_double * 4)(sigma, sigma, 0.0, sigma)
        fn = getattr(lib(), "blur_gaussian_%s_sigmas_pitched_batch_dev" % tname)
    else:
        sg = sigma
        fn = getattr(lib(), "blur_gaussian_%s_pitched_batch_dev" % tname)
    return fn(None, src, src_pitch, src_frame, dst, dst_pitch, dst_frame, nframes, rows, cols, ch, sg, C.byref(o))


@pytest.mark.parametrize("per_channel", [False, True], ids=["sigma", "sigmas"])
@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("tname", sorted(TYPES))
def test_bad_pitches_and_strides(tname, ch, per_channel):
    es = TYPES[tname]
    rowbytes = COLS * ch * es
    pitch = rowbytes + 8 * es
    span = (ROWS - 1) * pitch + rowbytes
    good = dict(tname=tname, per_channel=per_channel, src_pitch=pitch, src_frame=span, dst_pitch=pitch, dst_frame=span, ch=ch)
    # everything in order, no context: BLUR_ERR_INVALID for the missing context only (the same status as the packed entries give)
    assert call(**good) == INVALID
    # a pitch below a row's bytes, on either side
    assert call(**dict(good, src_pitch=rowbytes - es)) == INVALID
    assert call(**dict(good, dst_pitch=rowbytes - es)) == INVALID
    assert call(**dict(good, src_pitch=0)) == INVALID
    if es > 1:          # a pitch or a frame stride that is no multiple of the sample's size
        assert call(**dict(good, src_pitch=pitch + 1)) == INVALID
        assert call(**dict(good, dst_pitch=pitch + 1)) == INVALID
        assert call(**dict(good, src_frame=span + 1, nframes=2)) == INVALID
        assert call(**dict(good, dst_frame=span + 1, nframes=2)) == INVALID
    # several frames less than a frame's span apart
    assert call(**dict(good, src_frame=span - es, nframes=2)) == INVALID
    assert call(**dict(good, dst_frame=span - es, nframes=2)) == INVALID
    assert call(**dict(good, src_frame=0, dst_frame=0, nframes=3)) == INVALID


@pytest.mark.parametrize("per_channel", [False, True], ids=["sigma", "sigmas"])
@pytest.mark.parametrize("tname", sorted(TYPES))
def test_layout_errors_come_before_the_other_statuses(tname, per_channel):
    """a bad pitch is BLUR_ERR_INVALID even where the sigma alone would be BLUR_ERR_UNSUPPORTED; a good layout leaves the packed
    entries' statuses as they are (frame stride 0 with one frame is accepted)"""
    es = TYPES[tname]
    rowbytes = COLS * 3 * es
    assert call(tname, per_channel, rowbytes - es, 0, rowbytes, 0, sigma=30.0) == INVALID
    assert call(tname, per_channel, rowbytes, 0, rowbytes, 0, sigma=30.0) == UNSUPPORTED
    assert call(tname, per_channel, rowbytes + 64, 0, rowbytes + 128, 0, sigma=30.0) == UNSUPPORTED
    assert call(tname, per_channel, rowbytes + 64, 0, rowbytes + 128, 0) == INVALID            # only the context is missing
    for bad in (dict(ch=2), dict(rows=0), dict(cols=-1), dict(nframes=-1), dict(src=None), dict(dst=None)):
        assert call(tname, per_channel, rowbytes + 64, 0, rowbytes + 64, 0, **bad) == INVALID
    if not per_channel:
        assert call(tname, per_channel, rowbytes + 64, 0, rowbytes + 64, 0, sigma=0.0) == INVALID


def test_header_bindings_and_library_in_step():
    """every pitched entry is declared in the header, bound in _lib.SYMBOLS with the header's argument count, and exported"""
    from blur_algorithms_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "blur_amd.h")).read()
    L = lib()
    for tname in TYPES:
        for mid in ("", "_sigmas"):
            name = "blur_gaussian_%s%s_pitched_batch_dev" % (tname, mid)
            m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
            assert m, name
            assert name in _lib.SYMBOLS and hasattr(L, name)
            assert len(_lib.SYMBOLS[name][1]) == len(m.group(1).split(",")) == 13
            assert _lib.SYMBOLS[name][1][2:4] == [C.c_size_t, C.c_size_t] and _lib.SYMBOLS[name][1][5:7] == [C.c_size_t, C.c_size_t]


def layout(t):
    from blur_algorithms_amd.api import _gauss_strided_layout
    return _gauss_strided_layout(tuple(t.shape), tuple(t.stride()))


def test_strided_layout_accepts_pitched_views():
    import torch
    parent = torch.zeros(3, 40, 50, 4, dtype=torch.uint8)
    assert layout(parent) == (200, 8000)                                  # contiguous batch
    assert layout(parent[1]) == (200, 8000)                               # contiguous [R, Cc, C]
    assert layout(parent[1, 3:20, 5:30]) == (200, 17 * 200)               # ROI of [R, Cc, C]: one frame, rows a parent row apart
    assert layout(parent[:, 3:20, 5:30]) == (200, 8000)                   # ROI of a batch: frames a parent frame apart
    assert layout(parent[1:2, 3:20, 5:30]) == (200, 17 * 200)             # single-frame batch: its stride addresses nothing
    assert layout(parent[:, :, :17]) == (200, 8000)                       # padded rows (17 pixels in a 50-pixel pitch)
    grey = torch.zeros(40, 50, dtype=torch.float32)
    assert layout(grey) == (50, 2000)
    assert layout(grey[3:9, 5:20]) == (50, 6 * 50)                        # [rows, cols] ROI
    grey3 = torch.zeros(2, 40, 50, 1, dtype=torch.float32)
    assert layout(grey3[:, 3:9, 5:20]) == (50, 2000)
    # the smallest pitch and frame stride that still hold the rows and the frames
    from blur_algorithms_amd.api import _gauss_strided_layout
    assert _gauss_strided_layout((2, 6, 15, 3), (5 * 45 + 45, 45, 3, 1)) == (45, 270)


def test_strided_layout_refuses_everything_else():
    import torch
    from blur_algorithms_amd.api import _gauss_strided_layout
    parent = torch.zeros(3, 40, 50, 4, dtype=torch.uint8)
    assert layout(parent[..., :3]) is None                                # channel slices
    assert layout(parent[..., 1:2]) is None
    assert layout(parent[0, :, :, 2]) is None                             # one channel as a [rows, cols] image: pixels 4 apart
    assert layout(parent[:, :, ::2]) is None                              # stepped pixels
    assert layout(parent[..., ::2]) is None                               # stepped channels
    assert layout(parent.permute(0, 2, 1, 3)) is None                     # transposed
    assert layout(parent.permute(1, 0, 2, 3)) is None                     # frames inside the rows
    assert layout(parent.unsqueeze(0)) is None                            # five dimensions
    assert layout(torch.zeros(40, 50, 4, dtype=torch.uint8).expand(3, 40, 50, 4)) is None      # frame stride 0 with three frames
    # torch has no negative strides (flip copies); numpy-style flipped views, as strides
    assert _gauss_strided_layout((40, 50, 4), (-200, 4, 1)) is None       # rows flipped
    assert _gauss_strided_layout((40, 50, 4), (200, -4, 1)) is None       # pixels flipped
    assert _gauss_strided_layout((40, 50, 4), (200, 4, -1)) is None       # channels flipped
    assert _gauss_strided_layout((3, 40, 50, 4), (-8000, 200, 4, 1)) is None
    assert _gauss_strided_layout((40, 50, 4), (199, 4, 1)) is None        # rows overlap
    assert _gauss_strided_layout((3, 40, 50, 4), (7999, 200, 4, 1)) is None      # frames overlap
    assert _gauss_strided_layout((40, 50, 4), (200, 4)) is None


def test_multi_and_host_routes_keep_their_rules():
    """BlurMulti's helper call still demands contiguous frames (the layout is not analysed with a device given)"""
    import numpy as np
    import torch
    from blur_algorithms_amd.api import _gauss_tensor
    with pytest.raises(ValueError):
        _gauss_tensor(torch.zeros(2, 40, 50, 4, dtype=torch.uint8)[:, 3:20, 5:30], None, np.uint8, device=0)      # (a CPU tensor is refused anyway)
    with pytest.raises(ValueError):
        _gauss_tensor(torch.zeros(40, 50, 4, dtype=torch.uint8)[..., :3], None, np.uint8)
