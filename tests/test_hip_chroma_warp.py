"""GPU tests of the fused warps and the keep pass for 4:2:2 and 4:4:4 frames (functional.upsample_grid_sample_yuv, keep_borders_; C:
pws_upsample_grid_sample[_bicubic]_yuv_u8 / _u16, pws_border_keep_yuv_u8 / _u16) by PLANE EQUIVALENCE: the kernels' arithmetic depends on
nothing but a plane's own geometry, so every plane of a new-format frame must come out bit for bit as the same-sized plane of a 4:2:0 frame
does through the existing ``*_yuv420_*`` entry points (which tests/test_hip_yuv.py, test_hip_yuv16.py, test_hip_bicubic.py and
test_hip_keep.py hold to the float64 restatements).  tests/chroma_ref.py builds the carriers: the Y plane rides in a 4:2:0 frame of H x W,
4:2:2 chroma (H x W/2) in the chroma of a 4:2:0 frame of 2H x W in the same plane order, 4:4:4 chroma (H x W) in an I420 / I010 frame of
2H x 2W.  Whole frames are compared with ``==``, no tolerance.

Shapes (H, W, field size): keep_ref.SHAPES -- (16, 20, 8) chroma width 2 mod 4 at 4:2:2, (18, 24, 8) a partial last row group, (12, 520, 8)
rows across wave boundaries and a 4:4:4 chroma row that needs every 256-pixel chunk of the grid's y dimension -- plus (12, 520, 256), where
the field is read four corners per pixel in both planes (mode 0), and (720, 1280, 256) with 2 frames and align_corners=False: Y in the
wave-shared mode 2, 4:2:2 chroma in mode 3, 4:4:4 chroma in mode 2.  Fields: keep_ref.field_case's "shift", "outside" and "smooth" (pad
values, partially-outside taps, ragged rims).  T = 4; frames are uniform noise over all words."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chroma_ref as C  # noqa: E402
import keep_ref as K  # noqa: E402

NAMES = tuple(C.FORMATS)
SMALL = K.SHAPES + [(12, 520, 256)]
FIELDS = ("shift", "outside", "smooth")
MODES = ("bilinear", "bicubic")
_fields = {}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: cached arrays stay as they are)


def field_of(case, fs, n):
    """keep_ref.field_case, computed once per (case, size) and shared by every format."""
    if (case, fs) not in _fields:
        f = K.field_case(case, fs, seed=17)
        f.setflags(write=False)
        _fields[case, fs] = f
    return _fields[case, fs][:n]


def warp420(frames, field_d, fmt420, ac, mode):
    from pwstablenet_amd import functional as PF
    fn = PF.upsample_grid_sample_yuv420 if C.dtype(fmt420) == np.uint8 else PF.upsample_grid_sample_yuv420_16
    return fn(dev(frames), field_d, fmt420, align_corners=ac, mode=mode).cpu().numpy()


def check(fmt, n, h, w, fs, case, ac, mode, seed):
    """The warp of n noise frames, then the keep pass over the warped frames, against the carriers' 4:2:0 runs."""
    from pwstablenet_amd import functional as PF
    b = C.base420(fmt)
    field_d = dev(field_of(case, fs, n))
    f = C.random_frames(n, h, w, fmt, seed)
    got_d = PF.upsample_grid_sample_yuv(dev(f), field_d, fmt, align_corners=ac, mode=mode)
    got = got_d.cpu().numpy()
    assert got.shape == f.shape and got.dtype == f.dtype
    want = C.from_carriers(warp420(C.luma_carrier(f, fmt), field_d, b, ac, mode), warp420(C.chroma_carrier(f, fmt), field_d, b, ac, mode), fmt)
    assert np.array_equal(got, want), (fmt, h, w, fs, case, ac, mode, "warp")
    if case == "outside":   # BT.601 black exactly, in the format's placement
        y, u, v = C.unpack(got, fmt)
        deep, high = C.dtype(fmt) == np.uint16, C.ALL[fmt][1]
        black = [(16, 128), (64, 512), (64 << 6, 512 << 6)][deep + (deep and high)]
        assert (y == black[0]).all() and (u == black[1]).all() and (v == black[1]).all()
    else:
        assert not np.array_equal(got, f)
    init = C.random_frames(1, h, w, fmt, seed + 1)
    for source in (False, True):
        kept = PF.keep_borders_(got_d.clone(), field_d, dev(init[0]), fmt, initial_is_source=source, align_corners=ac, mode=mode).cpu().numpy()
        parts = []
        for carrier in (C.luma_carrier, C.chroma_carrier):
            parts.append(PF.keep_borders_(dev(carrier(got, fmt)), field_d, dev(carrier(init, fmt)[0]), b, initial_is_source=source, align_corners=ac,
                                          mode=mode).cpu().numpy())
        assert np.array_equal(kept, C.from_carriers(parts[0], parts[1], fmt)), (fmt, h, w, fs, case, ac, mode, "keep", source)
        if case == "outside":   # nothing is covered: every frame is the initial frame (as it is, or read as the warp writes it)
            assert (kept == kept[:1]).all() and (source or np.array_equal(kept[0], init[0]))
    return got


@pytest.mark.parametrize("hwf", SMALL, ids=lambda s: "%dx%d-f%d" % s)
@pytest.mark.parametrize("fmt", NAMES)
def test_planes_equal_the_420_planes(hip, fmt, hwf):
    h, w, fs = hwf
    for case in FIELDS:
        for mode in MODES:
            for ac in (False, True):
                check(fmt, K.T, h, w, fs, case, ac, mode, seed=h + w)


@pytest.mark.parametrize("fmt", NAMES)
def test_planes_equal_the_420_planes_720p(hip, fmt):
    h, w, fs = K.BIG
    for mode in MODES:
        check(fmt, 2, h, w, fs, "smooth", False, mode, seed=5)


@pytest.mark.parametrize("fmt420", ("nv12", "i420", "p010", "i010"))
def test_the_420_names_keep_their_bits(hip, fmt420):
    """upsample_grid_sample_yuv takes the 4:2:0 names too, and the new C entries with chroma = 0 are the old ones."""
    from pwstablenet_amd import functional as PF
    A = hip
    h, w, fs = 18, 24, 8
    f = C.random_frames(K.T, h, w, fmt420, seed=3)
    field_d = dev(field_of("smooth", fs, K.T))
    deep = C.dtype(fmt420) == np.uint16
    for mode in MODES:
        want = torch.from_numpy(warp420(f, field_d, fmt420, False, mode)).cuda()
        assert torch.equal(PF.upsample_grid_sample_yuv(dev(f), field_d, fmt420, mode=mode), want)
        out = torch.zeros_like(want)
        entry = "pws_upsample_grid_sample_%syuv_%s" % ("bicubic_" if mode == "bicubic" else "", "u16" if deep else "u8")
        A.check(getattr(A.lib(), entry)(A.ptr(dev(f)), A.ptr(field_d), A.ptr(out), K.T, h, w, fs, fs, PF.FRAME_FORMATS[fmt420].layout, 0, 0,
                                        A.current_stream()), entry)
        assert torch.equal(out, want)
    assert PF.yuv_shape(dev(f), fmt420) == (K.T, h, w)


def test_argument_checks(hip):
    from pwstablenet_amd import functional as PF
    A = hip
    lib, st = A.lib(), A.current_stream()
    field = torch.zeros((1, 4, 4, 2), device="cuda")
    u8 = torch.zeros((1, 24, 8), dtype=torch.uint8, device="cuda")
    u16 = torch.zeros((1, 24, 8), dtype=torch.uint16, device="cuda")
    for suffix, buf in (("u8", u8), ("u16", u16)):
        for entry in ("pws_upsample_grid_sample_yuv_" + suffix, "pws_upsample_grid_sample_bicubic_yuv_" + suffix):
            call = lambda h, w, layout, chroma: getattr(lib, entry)(A.ptr(buf), A.ptr(field), A.ptr(buf.clone()), 1, h, w, 4, 4, layout, chroma, 0, st)  # noqa: E731
            assert call(8, 8, 1, 2) == 0 and call(12, 8, 0, 1) == 0 and call(12, 8, 1, 1) == 0 and call(16, 8, 0, 0) == 0
            for h, w, layout, chroma, words in ((8, 8, 0, 2, "interleaved 4:4:4"), (8, 8, 1, 3, "chroma must be 0 (4:2:0), 1 (4:2:2) or 2 (4:4:4), got 3"),
                                                (8, 8, 1, -1, "chroma must be"), (8, 8, 2, 1, "layout must be 0"), (7, 8, 1, 2, "h must be even"),
                                                (8, 6, 1, 1, "w a multiple of 4")):
                assert call(h, w, layout, chroma) != 0
                assert entry + ": " in lib.pws_last_error().decode() and words in lib.pws_last_error().decode(), lib.pws_last_error().decode()
        keep = "pws_border_keep_yuv_" + suffix
        assert getattr(lib, keep)(A.ptr(buf.clone()), A.ptr(field), A.ptr(buf[0].clone()), 0, 1, 8, 8, 4, 4, 0, 2, 0, 0, st) != 0
        assert keep + ": interleaved 4:4:4" in lib.pws_last_error().decode()
    # the 4-tap window in the chroma planes: 4:2:2 needs w >= 8 like 4:2:0, 4:4:4 takes any valid w
    narrow = torch.zeros((1, 24, 4), dtype=torch.uint8, device="cuda")   # (H = 12 at 4:2:2, H = 8 at 4:4:4)
    assert PF.upsample_grid_sample_yuv(narrow, field, "i444", mode="bicubic").shape == narrow.shape
    assert PF.upsample_grid_sample_yuv(narrow, field, "nv16").shape == narrow.shape
    for name in ("nv16", "i422"):
        with pytest.raises(RuntimeError, match="w must be at least 8 \\(the chroma planes hold the 4-tap window\\), got 4"):
            PF.upsample_grid_sample_yuv(narrow, field, name, mode="bicubic")
        with pytest.raises(RuntimeError, match="w must be at least 8 with the bicubic margin, got 4"):
            PF.keep_borders_(narrow.clone(), field, narrow[0].clone(), name, mode="bicubic")
    assert PF.keep_borders_(narrow.clone(), field, narrow[0].clone(), "i444", mode="bicubic").shape == narrow.shape
    with pytest.raises(ValueError, match="i444 frames must be uint8"):
        PF.keep_borders_(u16, field, u16[0].clone(), "i444")
    with pytest.raises(RuntimeError):   # host frames
        PF.upsample_grid_sample_yuv(narrow.cpu(), field, "i444")
    assert PF.upsample_grid_sample_yuv(narrow[:0], field[:0], "i444").shape[0] == 0   # nothing to launch
