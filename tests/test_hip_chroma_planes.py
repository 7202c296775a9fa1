"""GPU tests of the window planes and the plane-wise output resize for 4:2:2 and 4:4:4 frames (stream.window_planes_yuv / _yuv16,
area_resize_yuv / _yuv16 with the names of functional.CHROMA_FORMATS; C: pws_gray_area_yuv_u8 / _u16, pws_area_resize_plane_u8 / _u16).

Window planes, bit for bit (torch.equal), at 258 x 260, 480 x 856 and 720 x 1280 (H x W):
  * a frame made by repeating a 4:2:0 frame's chroma (rows for 4:2:2, rows and columns for 4:4:4: chroma_ref.from420) shows that frame's
    picture, so its planes are ``window_planes_yuv`` / ``window_planes_yuv16`` of the 4:2:0 frame;
  * the planes of a frame whose chroma differs from sample to sample are ``stream.window_planes`` of the restatement's BGR decode
    (chroma_ref.yuv2bgr: the chroma of sample (x >> cx, y >> cy)), as test_hip_yuv.py::test_window_planes_yuv_equal_bgr_decode does it.
Area resize: against oracle/frameio_ref.resize_area_u8_hwc / yuv16_ref.resize_area_u10 plane by plane, as test_area_resize_yuv does it, on
the exact-half (64 x 48 -> 32 x 24), integer-ratio (96 x 72 -> 32 x 24) and table paths (258 x 260 -> (130, 128): the width halves, the
height does not), with an odd output height for 4:2:2 and an odd height and width for 4:4:4."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chroma_ref as C  # noqa: E402
import yuv16_ref as R16  # noqa: E402
import yuv_ref as R  # noqa: E402

NAMES = tuple(C.FORMATS)
SIZES = [(258, 260), (480, 856), (720, 1280)]   # (H, W)
_base = {}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def frames420(fmt420, h, w):
    """Two 4:2:0 frames, computed once per format and size: plausible samples, and noise over all words."""
    if (fmt420, h, w) not in _base:
        if C.dtype(fmt420) == np.uint8:
            f = np.concatenate([R.random_yuv(1, h, w, fmt420, seed=h + w), R.random_yuv(1, h, w, fmt420, seed=h, smooth=False)])
        else:
            f = np.concatenate([R16.random_yuv16(1, h, w, fmt420, seed=h + w), R16.random_yuv16(1, h, w, fmt420, seed=h, smooth=False)])
        f.setflags(write=False)
        _base[fmt420, h, w] = f
    return _base[fmt420, h, w]


def planes_of(frames, fmt):
    from pwstablenet_amd import stream as S
    fn = S.window_planes_yuv if C.dtype(fmt) == np.uint8 else S.window_planes_yuv16
    return fn(dev(frames), fmt, 256)


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fmt", NAMES)
def test_window_planes(hip, fmt, hw):
    from pwstablenet_amd import stream as S
    h, w = hw
    b = C.base420(fmt)
    f420 = frames420(b, h, w)
    # the 4:2:0 frame's picture
    got = planes_of(C.from420(f420, b, fmt), fmt)
    assert got.shape == (2, 256, 256) and got.dtype == torch.float32
    assert torch.equal(got, planes_of(f420, b))
    assert float(got[0].std()) > 0.05
    # chroma of its own in every sample: shifted copies of the Y plane's words as U and V (the same placement: plausible values in frame
    # 0, noise in frame 1, and no two neighbouring chroma samples tied to each other)
    y, _, _ = C.unpack(f420, b)
    cx, cy = C.shifts(fmt)
    u2, v2 = np.roll(y, 7, 2)[:, ::1 << cy, ::1 << cx], np.roll(y, 5, 1)[:, ::1 << cy, (1 << cx) - 1::1 << cx]
    f = C.pack(y, u2, v2, fmt)
    got = planes_of(f, fmt)
    assert torch.equal(got, S.window_planes(dev(C.yuv2bgr(f, fmt)), 256))
    assert not torch.equal(got, planes_of(f420, b))


def area_ref(frames, fmt, size):
    """cv2.resize(plane, INTER_AREA) plane by plane: Y to (height, width), chroma to (height >> cy, width >> cx), interleaved U V as a
    2-channel image; 16 bit on the 10-bit values, stored in the format's placement."""
    from oracle import frameio_ref
    ow, oh = size
    cx, cy = C.shifts(fmt)
    deep = C.dtype(fmt) == np.uint16
    y, u, v = ((C.samples10(p, fmt) if deep else p) for p in C.unpack(frames, fmt))
    rs = (lambda img, a, b: R16.resize_area_u10(img, a, b)) if deep else (lambda img, a, b: frameio_ref.resize_area_u8_hwc(img, a, b))
    ys = np.stack([rs(p[..., None], oh, ow)[..., 0] for p in y])
    if C.ALL[fmt][1]:
        c = np.stack([rs(np.stack([a, b], -1), oh >> cy, ow >> cx) for a, b in zip(u, v)])
        us, vs = c[..., 0], c[..., 1]
    else:
        us = np.stack([rs(p[..., None], oh >> cy, ow >> cx)[..., 0] for p in u])
        vs = np.stack([rs(p[..., None], oh >> cy, ow >> cx)[..., 0] for p in v])
    place = (lambda p: C.place10(p, fmt)) if deep else (lambda p: p)
    return C.pack(place(ys), place(us), place(vs), fmt)


#        source (H, W), output (width, height)
RESIZES = [((48, 64), (32, 24)), ((72, 96), (32, 24)), ((258, 260), (130, 128))]


@pytest.mark.parametrize("fmt", NAMES)
def test_area_resize(hip, fmt):
    from pwstablenet_amd import stream as S
    fn = S.area_resize_yuv if C.dtype(fmt) == np.uint8 else S.area_resize_yuv16
    mx, my = (1 << s for s in C.shifts(fmt))
    odd = [((48, 64), (32, 23))] if (mx, my) == (2, 1) else [((48, 64), (31, 23)), ((72, 96), (33, 25))]
    for (h, w), size in RESIZES + odd:
        f = C.random_frames(2, h, w, fmt, seed=h + size[0])
        got = fn(dev(f), fmt, size).cpu().numpy()
        assert got.shape == (2, C.packed_rows(fmt, size[1]), size[0]) and got.dtype == f.dtype
        assert np.array_equal(got, area_ref(f, fmt, size)), (fmt, h, w, size)
    f = dev(C.random_frames(1, 48, 64, fmt, seed=1))
    if mx == 2:   # 4:2:2: an odd width has no whole chroma sample
        with pytest.raises(ValueError, match="%s output size \\(31, 24\\) must be a multiple of 2 x 1" % fmt):
            fn(f, fmt, (31, 24))
    with pytest.raises(ValueError, match="within the 64 x 48 source"):
        fn(f, fmt, (66, 24))
    other = S.area_resize_yuv16 if C.dtype(fmt) == np.uint8 else S.area_resize_yuv
    with pytest.raises((ValueError, RuntimeError)):   # the other depth's wrapper does not take this name
        other(f, fmt, (32, 24))
