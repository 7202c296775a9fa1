"""CPU tests of the 4:2:2 / 4:4:4 formats: the numpy restatement tests/chroma_ref.py against the 4:2:0 restatements it extends, and the
record table functional.CHROMA_FORMATS with its shape rules and C entries.  No GPU and no library load."""
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chroma_ref as C  # noqa: E402
import yuv16_ref as R16  # noqa: E402
import yuv_ref as R  # noqa: E402

from pwstablenet_amd import functional as PF  # noqa: E402
from pwstablenet_amd import hipabi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nv16", "i422", "p210", "i210", "i444", "i410")
#        name: (dtype, layout, chroma, packed rows of H = 38)
TABLE = {"nv16": (torch.uint8, 0, 1, 76), "i422": (torch.uint8, 1, 1, 76), "p210": (torch.uint16, 0, 1, 76), "i210": (torch.uint16, 1, 1, 76),
         "i444": (torch.uint8, 1, 2, 114), "i410": (torch.uint16, 1, 2, 114)}


@pytest.mark.parametrize("fmt", NAMES)
def test_pack_unpack_round_trip(fmt):
    t, h, w = 2, 6, 8
    f = C.random_frames(t, h, w, fmt, seed=3)
    cx, cy = C.shifts(fmt)
    assert f.shape == (t, {1: 2 * h, 2: 3 * h}[C.ALL[fmt][2]], w) and f.dtype == C.dtype(fmt)
    y, u, v = C.unpack(f, fmt)
    assert y.shape == (t, h, w) and u.shape == v.shape == (t, h >> cy, w >> cx)
    assert np.array_equal(C.pack(y, u, v, fmt), f)
    # where the planes sit, written out: Y first; then U V pairs row by row, or the U plane and the V plane
    flat = f.reshape(t, -1)
    assert np.array_equal(flat[:, :h * w], y.reshape(t, -1))
    n = (h >> cy) * (w >> cx)
    if C.ALL[fmt][1]:
        assert np.array_equal(flat[:, h * w::2], u.reshape(t, -1)) and np.array_equal(flat[:, h * w + 1::2], v.reshape(t, -1))
    else:
        assert np.array_equal(flat[:, h * w:h * w + n], u.reshape(t, -1)) and np.array_equal(flat[:, h * w + n:], v.reshape(t, -1))
    # the carriers hold the planes they say, and give them back
    lum, chr_ = C.luma_carrier(f, fmt), C.chroma_carrier(f, fmt)
    b = C.base420(fmt)
    assert lum.shape == (t, h * 3 // 2, w) and chr_.shape == ((t, 3 * h, w) if C.ALL[fmt][2] == 1 else (t, 3 * h, 2 * w))
    assert np.array_equal(C.unpack(lum, b)[0], y)
    assert np.array_equal(C.unpack(chr_, b)[1], u) and np.array_equal(C.unpack(chr_, b)[2], v)
    assert np.array_equal(C.from_carriers(lum, chr_, fmt), f)


@pytest.mark.parametrize("fmt420", ("nv12", "i420"))
def test_the_420_packing_is_yuv_ref_s(fmt420):
    f = R.random_yuv(2, 6, 8, fmt420, seed=5, smooth=False)
    for a, b in zip(C.unpack(f, fmt420), R.unpack(f, fmt420)):
        assert np.array_equal(a, b)
    assert np.array_equal(C.pack(*R.unpack(f, fmt420), fmt420), f)


@pytest.mark.parametrize("fmt", NAMES)
def test_decode_of_repeated_chroma_is_the_420_decode(fmt):
    """A 4:2:2 frame made by repeating a 4:2:0 frame's chroma rows (a 4:4:4 frame: rows and columns) shows the same picture."""
    t, h, w = 2, 12, 16
    b = C.base420(fmt)
    if C.dtype(fmt) == np.uint8:
        f420 = R.random_yuv(t, h, w, b, seed=9, smooth=False)
        want = R.yuv2bgr(f420, b)
    else:   # (frame 0 plausible samples, frame 1 noise over all words: most I010 words of noise are above 1023 and decode as 255)
        f420 = np.concatenate([R16.random_yuv16(1, h, w, b, seed=9, noise=40), R16.random_yuv16(1, h, w, b, seed=9, smooth=False)])
        want = R.yuv2bgr(R16.reduce(f420, b), R16.FMT8[b])
    f = C.from420(f420, b, fmt)
    assert f.shape == (t, C.packed_rows(fmt, h), w)
    got = C.yuv2bgr(f, fmt)
    assert got.shape == (t, h, w, 3) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(C.yuv2bgr(f420, b), want)   # (and the general decode at 4:2:0 is yuv_ref's)
    assert len(np.unique(got)) > 100


def test_table():
    assert tuple(PF.CHROMA_FORMATS) == NAMES
    assert tuple(PF.FRAME_FORMATS) == ("bgr24", "nv12", "i420", "p010", "i010")   # still the five
    assert PF.PACKED_FORMATS == ("nv12", "i420", "p010", "i010") + NAMES
    for name, (dt, layout, chroma, rows) in TABLE.items():
        fmt = PF.CHROMA_FORMATS[name]
        assert PF.lookup_format(name) is fmt
        assert (fmt.name, fmt.dtype, fmt.packed, fmt.layout, fmt.chroma) == (name, dt, True, layout, chroma)
        assert fmt.packed_rows(38) == rows == C.packed_rows(name, 38)
        assert fmt.shifts == C.shifts(name) and fmt.multiples == (1 << fmt.shifts[0], 1 << fmt.shifts[1])
        assert fmt.args() == fmt.args(True) == (layout, chroma) and fmt.extra() == layout
        assert (np.uint8 if dt == torch.uint8 else np.uint16) == C.dtype(name)
        with pytest.raises(AttributeError):   # immutable
            fmt.chroma = 0
    for name, fmt in PF.FRAME_FORMATS.items():
        assert PF.lookup_format(name) is fmt
        assert fmt.chroma == (0 if fmt.packed else None)
        if fmt.packed:
            assert fmt.packed_rows(38) == 57 and fmt.shifts == (1, 1) and fmt.multiples == (2, 2) and fmt.args() == (fmt.layout,)
    assert PF.FRAME_FORMATS["bgr24"].args(True) == (1,)
    assert PF.lookup_format("nv24") is None and PF.lookup_format(None) is None and PF.lookup_format(["nv16"]) is None


@pytest.mark.parametrize("name", NAMES)
def test_entries_are_declared(name):
    fmt = PF.CHROMA_FORMATS[name]
    entries = [fmt.warp_entry(mode) for mode in PF.INTERPOLATIONS] + [fmt.keep_entry, fmt.window_planes, fmt.plane_resize]
    assert len(set(entries)) == 5
    header = open(os.path.join(ROOT, "include", "pwstable.h")).read()
    for entry in entries:
        assert entry in hipabi.SIGNATURES, entry
        assert re.search(r"^int %s\(" % entry, header, re.M), entry
    # the entries that take the chroma subsampling take one int more than their 4:2:0 twins, and are not those
    for entry in entries[:4]:
        twin = entry.replace("_yuv_", "_yuv420_")
        assert twin != entry and len(hipabi.SIGNATURES[entry][1]) == len(hipabi.SIGNATURES[twin][1]) + 1
    with pytest.raises(ValueError, match="mode must be one of"):
        fmt.warp_entry("nearest")


@pytest.mark.parametrize("name", NAMES)
def test_frame_shape(name):
    fmt = PF.CHROMA_FORMATS[name]
    rows = {1: "2 * H", 2: "3 * H"}[fmt.chroma]
    ph = {1: 76, 2: 114}[fmt.chroma]
    other = torch.uint16 if fmt.dtype == torch.uint8 else torch.uint8
    ok = torch.zeros((2, ph, 52), dtype=fmt.dtype)
    assert fmt.frame_shape(ok) == PF.yuv_shape(ok, name) == (2, 38, 52)
    assert PF.frame_format(name, ok, "run") is fmt
    assert fmt.frame_shape(torch.zeros((2, ph, 54), dtype=fmt.dtype), w_multiple=2) == (2, 38, 54)
    bad = [(torch.zeros((2, ph - 1, 52), dtype=fmt.dtype), 4, "%s frames: packed height %d is not %s of an even H" % (name, ph - 1, rows)),
           (torch.zeros((2, ph // 2, 52), dtype=fmt.dtype), 4, "%s frames: packed height %d is not %s of an even H" % (name, ph // 2, rows)),   # (H = 19)
           (torch.zeros((2, 0, 52), dtype=fmt.dtype), 4, "packed height 0 is not"),
           (torch.zeros((2, ph, 51), dtype=fmt.dtype), 4, "%s frames: width 51 must be even and a multiple of 4" % name),
           (torch.zeros((2, ph, 54), dtype=fmt.dtype), 4, "%s frames: width 54 must be even and a multiple of 4" % name),
           (torch.zeros((2, ph, 52, 3), dtype=fmt.dtype), 4, "%s frames must be %s (T, %s, W), got" % (name, str(fmt.dtype)[6:], rows)),
           (torch.zeros((2, ph, 52), dtype=other), 4, "%s frames must be %s (T, %s, W), got %s" % (name, str(fmt.dtype)[6:], rows, other))]
    for frames, multiple, fragment in bad:
        messages = []
        for call in (lambda: fmt.frame_shape(frames, multiple), lambda: PF.yuv_shape(frames, name, multiple)):
            with pytest.raises(ValueError) as e:
                call()
            assert fragment in str(e.value)
            messages.append(str(e.value))
        assert messages[0] == messages[1]
    with pytest.raises(ValueError, match="%s frames must be" % name):   # before any tensor is required on the device
        PF.frame_format(name, torch.zeros((2, ph, 52), dtype=other), "run")


def test_name_errors():
    u8 = torch.zeros((2, 76, 52), dtype=torch.uint8)
    field = torch.zeros((2, 8, 8, 2))
    for wrong in ("nv24", "p410", "bgr24", "yuv422p", None):
        with pytest.raises(ValueError, match="pixel_format must be one of .* for packed YUV frames, got"):
            PF.yuv_shape(u8, wrong)
        with pytest.raises(ValueError, match="pixel_format must be one of .* for packed YUV frames, got"):
            PF.upsample_grid_sample_yuv(u8, field, wrong)
    with pytest.raises(ValueError, match="mode must be one of"):   # (the mode comes first, as in the named wrappers)
        PF.upsample_grid_sample_yuv(u8, field, "nv24", mode="nearest")
    # the 4:2:0 wrappers stay 4:2:0-only, with their messages word for word
    for name in NAMES:
        with pytest.raises(ValueError) as e:
            PF.yuv420_layout(name)
        assert str(e.value) == ("pixel_format must be one of ('nv12', 'i420') for 4:2:0 frames, got %r (8-bit BT.601 limited-range NV12 / I420 only)" % name)
        with pytest.raises(ValueError) as e:
            PF.yuv420_16_shape(u8, name)
        assert str(e.value) == ("pixel_format must be one of ('p010', 'i010') for 10-bit 4:2:0 frames, got %r (BT.601 limited-range P010 / I010 only)"
                                % name)
        with pytest.raises(ValueError, match="for 4:2:0 frames"):
            PF.yuv420_shape(u8, name)
        with pytest.raises(ValueError, match="for 10-bit 4:2:0 frames"):   # (this wrapper resolves the name before it asks for device tensors)
            PF.upsample_grid_sample_yuv420_16(u8, field, name)
    with pytest.raises(ValueError, match="pixel_format must be one of"):   # (an unknown name under run / keep_borders_: yuv420_layout's error)
        PF.frame_format("nv24", u8, "run")
    # shape errors win over host tensors in the generic wrapper, as in upsample_grid_sample_yuv420_16
    with pytest.raises(ValueError, match="nv16 frames: packed height 75"):
        PF.upsample_grid_sample_yuv(torch.zeros((2, 75, 52), dtype=torch.uint8), field, "nv16")
    with pytest.raises(ValueError, match="i410 frames must be uint16"):
        PF.upsample_grid_sample_yuv(u8, field, "i410")
    # the stream wrappers take the names of their depth only
    from pwstablenet_amd import stream as S
    assert S._yuv_format("i444", torch.uint8) is PF.CHROMA_FORMATS["i444"] and S._yuv_format("p210", torch.uint16) is PF.CHROMA_FORMATS["p210"]
    with pytest.raises(ValueError, match="for 4:2:0 frames"):
        S._yuv_format("p210", torch.uint8)
    with pytest.raises(ValueError, match="for 10-bit 4:2:0 frames"):
        S._yuv_format("i444", torch.uint16)
    assert S._frames_shape(PF.CHROMA_FORMATS["i422"], 3, 38, 52) == (3, 76, 52) and S._frames_shape(PF.CHROMA_FORMATS["i410"], 3, 37, 51) == (3, 111, 51)
    assert S._frames_shape(PF.FRAME_FORMATS["nv12"], 3, 38, 52) == (3, 57, 52) and S._frames_shape(PF.FRAME_FORMATS["bgr24"], 3, 38, 52) == (3, 38, 52, 3)


@pytest.mark.parametrize("name", ("nv12", "i010") + NAMES)
def test_plane_views_and_crop_on_the_host(name):
    """FrameFormat.planes and stream._yuv_crop against the restatement's packing (host tensors: views and copies only)."""
    from pwstablenet_amd import stream as S
    fmt = PF.lookup_format(name)
    t, h, w = 2, 12, 16
    f = C.random_frames(t, h, w, name, seed=4)
    as_t = lambda a: torch.from_numpy(a.astype(np.int32))   # noqa: E731  (values only; uint16 tensors have few host operators)
    planes = fmt.planes(as_t(f), h, w)
    y, u, v = C.unpack(f, name)
    assert np.array_equal(planes[0].numpy(), y)
    if fmt.layout == 0:
        assert len(planes) == 2 and np.array_equal(planes[1].numpy(), np.stack([u, v], -1).reshape(t, u.shape[1], -1))
    else:
        assert len(planes) == 3 and np.array_equal(planes[1].numpy(), u) and np.array_equal(planes[2].numpy(), v)
    mx, my = fmt.multiples
    y0, y1, x0, x1 = my, h - 3 * my, 3 * mx, w - mx   # (odd edges wherever the format allows them)
    cx, cy = fmt.shifts
    got = S._yuv_crop(as_t(f), h, w, name, y0, y1, x0, x1).numpy()
    want = C.pack(y[:, y0:y1, x0:x1], u[:, y0 >> cy:y1 >> cy, x0 >> cx:x1 >> cx], v[:, y0 >> cy:y1 >> cy, x0 >> cx:x1 >> cx], name)
    assert got.shape == want.shape and np.array_equal(got, want)
