"""blur_gaussian_nv12_* and blur_gaussian_p016_* (decoded video surfaces: a luma plane and a half-resolution plane of interleaved
Cb/Cr pairs): the statuses that need no device (the checks run before the context is touched, so ctx may be NULL), the bindings, the
Python wrapper's checks and scalar-sigma rule on CPU tensors, and the layout helper api._nv12_layout on strides."""
import ctypes as C
import os
import re

import numpy as np
import pytest

INVALID, UNSUPPORTED = 1, 2
KINDS = {"nv12": 1, "p016": 2}          # entry name -> bytes per sample
ROWS, COLS = 40, 92                     # luma; chroma 20 x 46


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
NAN, INF = float("nan"), float("inf")


def pad_of(rows, cols, sigma):
    import blur_algorithms_amd as B
    return B.pffft_sizing(rows, cols, sigma)["pad"]


def good(kind, rows=ROWS, cols=COLS):
    es = KINDS[kind]
    pitch = (cols + 8) * es
    return dict(kind=kind, sy=P, suv=P, spitch=pitch, sys=rows * pitch, suvs=rows // 2 * pitch, dy=P, duv=P, dpitch=pitch, dys=rows * pitch,
                duvs=rows // 2 * pitch, nframes=1, rows=rows, cols=cols, sigmas=(2.0, 1.0, 1.0))


def call(entry, kind, sy, suv, spitch, sys, suvs, dy, duv, dpitch, dys, duvs, nframes, rows, cols, sigmas):
    """entry: batch_dev, dev (one frame: no frame strides, nframes ignored) or host (packed: no pitches, sy and dy only)"""
    o = opts()
    sg = None if sigmas is None else (C.c_double * 3)(*sigmas)
    fn = getattr(lib(), "blur_gaussian_%s_%s" % (kind, entry))
    if entry == "batch_dev":
        return fn(None, sy, suv, spitch, sys, suvs, dy, duv, dpitch, dys, duvs, nframes, rows, cols, sg, C.byref(o))
    if entry == "dev":
        return fn(None, sy, suv, spitch, dy, duv, dpitch, rows, cols, sg, C.byref(o))
    return fn(None, sy, dy, rows, cols, sg, C.byref(o))


ENTRIES = ("batch_dev", "dev", "host")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_pointers_sizes_and_sigmas(kind, entry):
    g = good(kind)
    # everything in order, no context: BLUR_ERR_INVALID for the missing context only
    assert call(entry, **g) == INVALID
    bad = [dict(sy=None), dict(dy=None), dict(sigmas=None), dict(rows=0), dict(cols=0), dict(rows=-2), dict(cols=-2), dict(rows=ROWS + 1), dict(cols=COLS + 1),
           dict(rows=1), dict(sigmas=(-1.0, 1.0, 1.0)), dict(sigmas=(2.0, NAN, 1.0)), dict(sigmas=(2.0, 1.0, INF)), dict(sigmas=(2.0, 1.0, -0.5))]
    if entry != "host":
        bad += [dict(suv=None), dict(duv=None)]
    if entry == "batch_dev":
        bad += [dict(nframes=-1)]
    for b in bad:
        assert call(entry, **dict(g, **b)) == INVALID, b
    # sigma = 0 is a plane or channel left as it is, not an error (only the context is missing); and so are all three
    assert call(entry, **dict(g, sigmas=(0.0, 1.0, 0.0))) == INVALID
    assert call(entry, **dict(g, sigmas=(0.0, 0.0, 0.0))) == INVALID


@pytest.mark.parametrize("entry", ["batch_dev", "dev"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_pitches_and_strides(kind, entry):
    es = KINDS[kind]
    g = good(kind)
    rowbytes = COLS * es
    assert call(entry, **dict(g, spitch=rowbytes, dpitch=rowbytes)) == INVALID           # the packed surface: only the context is missing
    for side in ("spitch", "dpitch"):
        assert call(entry, **dict(g, **{side: rowbytes - es})) == INVALID
        assert call(entry, **dict(g, **{side: 0})) == INVALID
        if es > 1:
            assert call(entry, **dict(g, **{side: g[side] + 1})) == INVALID
    if entry != "batch_dev":
        return
    pitch = g["spitch"]
    yspan, uvspan = (ROWS - 1) * pitch + rowbytes, (ROWS // 2 - 1) * pitch + rowbytes
    two = dict(g, nframes=2, sys=yspan, dys=yspan, suvs=uvspan, duvs=uvspan)
    assert call(entry, **two) == INVALID                                                   # the smallest strides: only the context is missing
    for key, span in (("sys", yspan), ("dys", yspan), ("suvs", uvspan), ("duvs", uvspan)):
        assert call(entry, **dict(two, **{key: span - es})) == INVALID, key
        assert call(entry, **dict(two, **{key: 0})) == INVALID, key
        if es > 1:
            assert call(entry, **dict(two, **{key: span + 1})) == INVALID, key
    # a chroma stride that would do for the luma's rows is not asked of the chroma plane, and the reverse is refused
    assert call(entry, **dict(two, sys=uvspan)) == INVALID
    # one frame: its strides address nothing and are not looked at
    assert call(entry, **dict(g, sys=1, suvs=3, dys=5, duvs=7)) == INVALID
    # no frames: still checked, then a no-op for a context
    assert call(entry, **dict(g, nframes=0, rows=ROWS + 1)) == INVALID


def status_with_sigmas(entry, kind, rows, cols, sigmas, **kw):
    return call(entry, **dict(good(kind, rows, cols), sigmas=sigmas, **kw))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_pad_limits_per_plane(kind, entry):
    """each sigma is in pixels of its own plane: one that fits the luma plane and not the chroma plane is BLUR_ERR_UNSUPPORTED as
    sigmas[1] or sigmas[2] and accepted as sigmas[0]"""
    s = 7.0
    p_luma, p_chroma = pad_of(ROWS, COLS, s), pad_of(ROWS // 2, COLS // 2, s)
    assert p_luma <= min(ROWS, COLS) - 1 and p_chroma > min(ROWS // 2, COLS // 2) - 1, (p_luma, p_chroma)
    assert status_with_sigmas(entry, kind, ROWS, COLS, (s, 1.0, 1.0)) == INVALID          # accepted: only the context is missing
    assert status_with_sigmas(entry, kind, ROWS, COLS, (1.0, s, 1.0)) == UNSUPPORTED
    assert status_with_sigmas(entry, kind, ROWS, COLS, (1.0, 1.0, s)) == UNSUPPORTED
    assert status_with_sigmas(entry, kind, ROWS, COLS, (0.0, 0.0, s)) == UNSUPPORTED
    big = 30.0
    assert pad_of(ROWS, COLS, big) > min(ROWS, COLS) - 1
    assert status_with_sigmas(entry, kind, ROWS, COLS, (big, 1.0, 1.0)) == UNSUPPORTED
    # the largest pad a plane holds is its smaller side less one
    for rows, cols in ((ROWS, COLS), (COLS, ROWS)):
        edge = min(rows, cols) // 2 - 1
        se = next(x / 100.0 for x in range(50, 3000) if pad_of(rows // 2, cols // 2, x / 100.0) == edge)
        so = next(x / 100.0 for x in range(50, 3000) if pad_of(rows // 2, cols // 2, x / 100.0) == edge + 1)
        assert status_with_sigmas(entry, kind, rows, cols, (1.0, se, se)) == INVALID
        assert status_with_sigmas(entry, kind, rows, cols, (1.0, se, so)) == UNSUPPORTED


@pytest.mark.parametrize("entry", ["batch_dev", "dev"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_layout_errors_come_before_unsupported(kind, entry):
    es = KINDS[kind]
    big = (30.0, 1.0, 1.0)
    assert status_with_sigmas(entry, kind, ROWS, COLS, big) == UNSUPPORTED
    assert status_with_sigmas(entry, kind, ROWS, COLS, big, spitch=COLS * es - es) == INVALID
    assert status_with_sigmas(entry, kind, ROWS, COLS, big, dpitch=COLS * es - es) == INVALID
    assert status_with_sigmas(entry, kind, ROWS + 1, COLS, big) == INVALID
    assert status_with_sigmas(entry, kind, ROWS, COLS, (30.0, -1.0, 1.0)) == INVALID
    if entry == "batch_dev":
        assert status_with_sigmas(entry, kind, ROWS, COLS, big, nframes=2, suvs=8) == INVALID
        assert status_with_sigmas(entry, kind, ROWS, COLS, big, nframes=2) == UNSUPPORTED


def test_two_channels_stay_illegal_in_every_public_entry():
    """the chroma plane's channel count is legal inside the NV12 / P016 driver only"""
    o = opts()
    sg = (C.c_double * 4)(2.0, 2.0, 2.0, 2.0)
    L = lib()
    for t, es in (("u8", 1), ("u16", 2), ("f32", 4)):
        pitch = COLS * 2 * es
        assert getattr(L, "blur_gaussian_%s_batch_dev" % t)(None, P, P, 1, ROWS, COLS, 2, 2.0, C.byref(o)) == INVALID
        assert getattr(L, "blur_gaussian_%s_sigmas_batch_dev" % t)(None, P, P, 1, ROWS, COLS, 2, sg, C.byref(o)) == INVALID
        assert getattr(L, "blur_gaussian_%s_pitched_batch_dev" % t)(None, P, pitch, 0, P, pitch, 0, 1, ROWS, COLS, 2, 30.0, C.byref(o)) == INVALID
        assert getattr(L, "blur_gaussian_%s_sigmas_pitched_batch_dev" % t)(None, P, pitch, 0, P, pitch, 0, 1, ROWS, COLS, 2, sg, C.byref(o)) == INVALID
    out = (C.c_int * 6)()
    assert L.blur_gaussian_sigmas_plan(ROWS, COLS, 2, sg, out) == INVALID


def test_header_bindings_and_library_in_step():
    from blur_algorithms_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "blur_amd.h")).read()
    L = lib()
    for kind in KINDS:
        for entry, nargs in (("batch_dev", 16), ("dev", 11), ("host", 7)):
            name = "blur_gaussian_%s_%s" % (kind, entry)
            m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
            assert m, name
            assert name in _lib.SYMBOLS and hasattr(L, name)
            assert len(_lib.SYMBOLS[name][1]) == len(m.group(1).split(",")) == nargs
    sz = [C.c_size_t] * 3
    for kind in KINDS:
        args = _lib.SYMBOLS["blur_gaussian_%s_batch_dev" % kind][1]
        assert args[3:6] == sz and args[8:11] == sz
    hpp = open(os.path.join(here, "..", "include", "blur_amd.hpp")).read()
    assert "gaussian_blur_nv12_dev(" in hpp and "gaussian_blur_p016_dev(" in hpp


# ---- the layout helper, on strides ---------------------------------------------------------------------------------------------
def layout(*a):
    from blur_algorithms_amd.api import _nv12_layout
    return _nv12_layout(*a)


def test_layout_of_surfaces_and_views():
    R, Cc, Pi = 40, 92, 128
    # one frame: contiguous planes, and the two planes of a pitched surface
    assert layout((R, Cc), (Cc, 1), (R // 2, Cc // 2, 2), (Cc, 2, 1)) == (1, R, Cc, Cc, R * Cc, R // 2 * Cc)
    assert layout((R, Cc), (Pi, 1), (R // 2, Cc // 2, 2), (Pi, 2, 1)) == (1, R, Cc, Pi, R * Pi, R // 2 * Pi)
    # batches: each plane has its own frame stride (UV behind Y in every surface; Y and UV in two allocations)
    surf = 64 * Pi
    assert layout((3, R, Cc), (surf, Pi, 1), (3, R // 2, Cc // 2, 2), (surf, Pi, 2, 1)) == (3, R, Cc, Pi, surf, surf)
    assert layout((3, R, Cc), (R * Pi, Pi, 1), (3, R // 2, Cc // 2, 2), (R // 2 * Pi + 7, Pi, 2, 1)) == (3, R, Cc, Pi, R * Pi, R // 2 * Pi + 7)
    # the smallest frame strides that hold the planes
    ys, uvs = (R - 1) * Pi + Cc, (R // 2 - 1) * Pi + Cc
    assert layout((2, R, Cc), (ys, Pi, 1), (2, R // 2, Cc // 2, 2), (uvs, Pi, 2, 1)) == (2, R, Cc, Pi, ys, uvs)
    # a batch of one: its frame strides address nothing
    assert layout((1, R, Cc), (5, Pi, 1), (1, R // 2, Cc // 2, 2), (3, Pi, 2, 1)) == (1, R, Cc, Pi, R * Pi, R // 2 * Pi)
    # two luma rows: the one chroma row's pitch addresses nothing; two luma columns: one Cb/Cr pair per row
    assert layout((2, Cc), (Pi, 1), (1, Cc // 2, 2), (999, 2, 1)) == (1, 2, Cc, Pi, 2 * Pi, Pi)
    assert layout((R, 2), (Pi, 1), (R // 2, 1, 2), (Pi, 77, 1)) == (1, R, 2, Pi, R * Pi, R // 2 * Pi)


@pytest.mark.parametrize("args", [
    ((41, 92), (92, 1), (20, 46, 2), (92, 2, 1)),                  # odd rows
    ((40, 93), (93, 1), (20, 46, 2), (93, 2, 1)),                  # odd cols
    ((40, 92), (92, 1), (20, 45, 2), (92, 2, 1)),                  # chroma of another width
    ((40, 92), (92, 1), (40, 46, 2), (92, 2, 1)),                  # full-height chroma
    ((40, 92), (92, 1), (20, 46, 3), (138, 3, 1)),                 # three samples per chroma pixel
    ((40, 92), (92, 1), (20, 92), (92, 1)),                        # chroma rows not split into pairs
    ((2, 40, 92), (3680, 92, 1), (3, 20, 46, 2), (1840, 92, 2, 1)),        # another number of frames
    ((40, 92), (128, 1), (20, 46, 2), (256, 2, 1)),                # unequal pitches
    ((40, 92), (128, 1), (20, 46, 2), (92, 2, 1)),
    ((40, 92), (91, 1), (20, 46, 2), (91, 2, 1)),                  # rows overlap
    ((40, 92), (-128, 1), (20, 46, 2), (-128, 2, 1)),              # rows flipped
    ((40, 92), (128, 2), (20, 46, 2), (128, 2, 1)),                # stepped luma samples
    ((40, 92), (128, 1), (20, 46, 2), (128, 4, 1)),                # stepped pairs
    ((40, 92), (128, 1), (20, 46, 2), (128, 2, -1)),               # Cr before Cb
    ((40, 92), (1, 40), (20, 46, 2), (92, 2, 1)),                  # transposed
    ((2, 40, 92), (5000, 128, 1), (2, 20, 46, 2), (2000, 128, 2, 1)),      # chroma frames overlap
    ((2, 40, 92), (0, 128, 1), (2, 20, 46, 2), (0, 128, 2, 1)),            # frame stride 0 with two frames
    ((1, 2, 40, 92), (1, 1, 92, 1), (1, 2, 20, 46, 2), (1, 1, 92, 2, 1)),  # too many dimensions
    ((0, 92), (92, 1), (0, 46, 2), (92, 2, 1)),
])
def test_layout_refuses_everything_else(args):
    with pytest.raises(ValueError):
        layout(*args)


# ---- the wrapper's checks, on CPU tensors (no context is needed: they run before the library is called) ------------------------------
def tensors(y, uv, out=None, **kw):
    from blur_algorithms_amd.api import _nv12_tensors
    return _nv12_tensors(y, uv, out, **kw)


def test_wrapper_accepts_the_planes_of_a_surface():
    import torch
    for dt in (torch.uint8, torch.uint16):
        surf = torch.zeros(64, 128, dtype=dt)                                # 40 luma rows, 2 rows of padding, 20 chroma rows
        y, uv = surf[:40, :92], surf[42:62, :92].unflatten(-1, (46, 2))
        assert not y.is_contiguous() and not uv.is_contiguous()
        r = tensors(y, uv, require_cuda=False)
        assert r[4] == r[5] == (1, 40, 92, 128, 40 * 128, 20 * 128) and r[2] is y and r[3] is uv         # in place by default
        yo, uvo = torch.zeros(40, 92, dtype=dt), torch.zeros(20, 46, 2, dtype=dt)
        r = tensors(y, uv, (yo, uvo), require_cuda=False)
        assert r[4][3] == 128 and r[5] == (1, 40, 92, 92, 40 * 92, 20 * 92) and r[2] is yo and r[3] is uvo
        batch = torch.zeros(3, 64, 128, dtype=dt)
        r = tensors(batch[:, :40, :92], batch[:, 42:62, :92].unflatten(-1, (46, 2)), require_cuda=False)
        assert r[4] == (3, 40, 92, 128, 64 * 128, 64 * 128)


def test_wrapper_refuses_before_the_library_is_called():
    import torch
    y, uv = torch.zeros(40, 92, dtype=torch.uint8), torch.zeros(20, 46, 2, dtype=torch.uint8)
    with pytest.raises(ValueError):
        tensors(y, uv)                                                       # CPU tensors (the numpy route is the host route)
    bad = [(y, uv.to(torch.uint16)), (y.to(torch.uint16), uv), (y.float(), uv.float()), (y.to(torch.int16), uv.to(torch.int16)),
           (y[:39], uv), (y[:, :91], uv), (y, uv[:19]), (y, uv[:, :45]), (y, torch.zeros(20, 92, dtype=torch.uint8)),
           (torch.zeros(40, 128, dtype=torch.uint8)[:, :92], uv),                                    # unequal pitches
           (y.t().contiguous().t(), uv),                                                             # column-major luma
           (torch.zeros(40, 184, dtype=torch.uint8)[:, ::2], uv),                                    # stepped luma samples
           (y, torch.zeros(20, 46, 4, dtype=torch.uint8)[..., :2]),                                  # a channel slice of a wider chroma plane
           (y, uv.permute(1, 0, 2))]
    for a, b in bad:
        with pytest.raises(ValueError):
            tensors(a, b, require_cuda=False)
    outs = [(y,), (y, uv, y), y, (y, uv.to(torch.uint16)), (y[:38], uv), (torch.zeros(40, 92, dtype=torch.uint8), torch.zeros(20, 46, 3, dtype=torch.uint8)),
            (torch.zeros(40, 128, dtype=torch.uint8)[:, :92], torch.zeros(20, 46, 2, dtype=torch.uint8))]                 # the last: unequal pitches in `out`
    for out in outs:
        with pytest.raises(ValueError):
            tensors(y, uv, out, require_cuda=False)


def test_scalar_sigma_is_the_same_blur_in_luma_pixels():
    from blur_algorithms_amd.api import _nv12_sigmas
    assert _nv12_sigmas(20) == (20.0, 10.0, 10.0)
    assert _nv12_sigmas(3.0) == (3.0, 1.5, 1.5)
    assert _nv12_sigmas(np.float32(5)) == (5.0, 2.5, 2.5)
    assert _nv12_sigmas(np.array(4.0)) == (4.0, 2.0, 2.0)                    # a 0-d array is a scalar
    assert _nv12_sigmas((1, 11, 11)) == (1.0, 11.0, 11.0)                    # a sequence is taken as given
    assert _nv12_sigmas([0, 5, 7]) == (0.0, 5.0, 7.0)
    assert _nv12_sigmas(np.array([5.0, 5.0, 7.0])) == (5.0, 5.0, 7.0)
    for bad in ((1, 2), (1, 2, 3, 4), [], [5.0]):
        with pytest.raises(ValueError):
            _nv12_sigmas(bad)


def test_method_exists_with_the_documented_signature():
    import inspect
    import blur_algorithms_amd as B
    sig = inspect.signature(B.BlurContext.gaussian_nv12)
    assert list(sig.parameters) == ["self", "y", "uv", "sigma", "out", "nyquist_quirk", "engine"]
    assert sig.parameters["out"].default is None and sig.parameters["nyquist_quirk"].default is True and sig.parameters["engine"].default is None
