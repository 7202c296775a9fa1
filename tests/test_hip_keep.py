"""GPU tests of the "keep" borders kernel (csrc/border_keep.hip; functional.keep_borders_, C: pws_border_keep_u8 / _yuv420_u8 / _yuv420_u16)
against the float64 restatement tests/keep_ref.py.

Every format (bgr24 with and without swap_rb, nv12, i420, p010, i010) x both align_corners values x both margins (bilinear 0, bicubic 1) x
four fields (keep_ref.field_case: identity, a shift that uncovers a wedge on two sides, everything outside, a smooth random field) at 16 x 20
(chroma width 10 = 2 mod 4), 18 x 24 (odd chroma height) and 12 x 520 (rows that cross wave boundaries) with 8 x 8 fields, and one 720 x 1280
case per format with a 256 x 256 field (the wave-shared field modes); T = 4 frames, the initial frame once as a source frame (read rules
applied) and once as an earlier output frame.  The frames hold random bytes / words: the kernel copies, and only equality is checked.

Check, frame by frame: where a pixel's float64 coordinates lie further than delta from every coverage threshold, out[t] EQUALS
covered ? warped[t] : out[t-1] (out[t-1] being the device's own previous frame, or the initial frame under its read rules); elsewhere either
of the two values is accepted; no sample is ever anything else.

delta is derived on the CPU, per plane, as 4 x the largest distance between the kernels' fp32 coordinate sequence evaluated in numpy float32
(keep_ref.coordinates32) and the float64 coordinates on that very field; the factor 4 leaves room for another order of operations in the
field's interpolation.  Measured (tests/test_keep_ref_cpu.py prints them): the largest fp32 error is 6.4e-4 pixels (720 x 1280 Y plane, smooth
field, align_corners=True), so delta <= 2.6e-3 pixels there; 2.5e-4 / 1.0e-3 on the 360 x 640 chroma planes; at most 7.7e-5 / 3.1e-4 on the
small shapes.  (The all-outside field has coordinates of ~1e4 plane widths and an error of ~1 pixel; every distance there is ~1e7.)
The CPU test holds every field used here to at most 1 % of undecided pixels per plane by the restatement alone (measured: 0.19 % at most)."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keep_ref as K  # noqa: E402

FORMATS = ["bgr24", "bgr24-swap", "nv12", "i420", "p010", "i010"]
MODES = ["bilinear", "bicubic"]
# the 720 x 1280 case of each format: (field, align_corners, mode) -- two combinations, so the float64 reference is computed twice in all
BIG_A, BIG_B = ("smooth", False, "bilinear"), ("shift", True, "bicubic")
BIG_CASE = {"bgr24": BIG_A, "bgr24-swap": BIG_B, "nv12": BIG_A, "i420": BIG_B, "p010": BIG_B, "i010": BIG_A}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the cached fields are read-only)


@functools.lru_cache(maxsize=None)
def field_of(case, fs, seed):
    f = K.field_case(case, fs, seed)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def plane_ref(case, fs, seed, ph, pw, ac, m):
    """(covered, decided) of one plane, computed once per case and shared by the formats: decided = further than delta from every threshold."""
    field = field_of(case, fs, seed)
    delta = K.FACTOR * K.fp32_error(field, ph, pw, ac)
    cov, dist = K.coverage(field, ph, pw, ac, m)
    return cov, dist > delta


def packed_ref(fmt, case, fs, seed, h, w, ac, m):
    cy, dy = plane_ref(case, fs, seed, h, w, ac, m)
    if fmt == "bgr24":
        return np.repeat(cy[..., None], 3, -1), np.repeat(dy[..., None], 3, -1)
    cc, dc = plane_ref(case, fs, seed, h // 2, w // 2, ac, m)
    return K._pack(cy, cc, fmt), K._pack(dy, dc, fmt)


def run_case(fmt_name, h, w, fs, case, ac, mode):
    from pwstablenet_amd import functional as PF
    fmt, swap = fmt_name.split("-")[0], fmt_name.endswith("swap")
    m = K.margin(mode)
    field = field_of(case, fs, w)
    cov, decided = packed_ref(fmt, case, fs, w, h, w, ac, m)
    share = 1 - decided.mean()
    assert share <= K.CAP, share
    rs = np.random.RandomState(h * 7 + w + len(fmt_name))
    deep = fmt in K.YUV16
    shape = (K.T, h, w, 3) if fmt == "bgr24" else (K.T, h * 3 // 2, w)
    draw = lambda s: rs.randint(0, 65536 if deep else 256, s).astype(np.uint16 if deep else np.uint8)   # noqa: E731
    warped, init = draw(shape), draw(shape[1:])   # (any words: junk in P010's low bits, I010 words above 1023)
    field_d = dev(field)
    for source in (True, False):
        buf = dev(warped)
        got = PF.keep_borders_(buf, field_d, dev(init), fmt, initial_is_source=source, swap_rb=swap, align_corners=ac, mode=mode)
        assert got is buf   # in place
        got = got.cpu().numpy()
        first = K.initial_frame(init, fmt, source, swap)
        prev = first
        for t in range(K.T):
            assert ((got[t] == warped[t]) | (got[t] == prev)).all(), (fmt_name, case, ac, mode, t)   # never a third value
            want = K.step(prev, warped[t], cov[t])
            bad = (got[t] != want) & decided[t]
            assert not bad.any(), (fmt_name, case, ac, mode, source, t, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            prev = got[t]
        if case == "identity" and mode == "bilinear":
            assert np.array_equal(got, warped)
        if case == "outside":
            assert all(np.array_equal(got[t], first) for t in range(K.T))
        if case in ("shift", "smooth"):
            assert not np.array_equal(got, warped)
    return share


@pytest.mark.parametrize("hwf", K.SHAPES, ids=lambda s: "%dx%d" % (s[0], s[1]))
@pytest.mark.parametrize("fmt", FORMATS)
def test_keep_small(hip, fmt, hwf):
    h, w, fs = hwf
    worst = 0.0
    for case in K.FIELDS:
        for ac in (False, True):
            for mode in MODES:
                worst = max(worst, run_case(fmt, h, w, fs, case, ac, mode))
    print("%s %dx%d: largest share of undecided samples %.4f" % (fmt, h, w, worst))


@pytest.mark.parametrize("fmt", FORMATS)
def test_keep_720p(hip, fmt):
    h, w, fs = K.BIG
    case, ac, mode = BIG_CASE[fmt]
    print("%s 720p %s ac=%s %s: share of undecided samples %.5f" % (fmt, case, ac, mode, run_case(fmt, h, w, fs, case, ac, mode)))


def test_read_rules_of_a_source_frame(hip):
    """Everything outside: every frame becomes the initial frame -- swapped, masked or clamped when it is a source frame, as it is otherwise."""
    from pwstablenet_amd import functional as PF
    h, w = 16, 20
    field = dev(K.field_case("outside", 8, 0))
    rs = np.random.RandomState(3)
    for fmt, swap in (("bgr24", True), ("bgr24", False), ("nv12", False), ("i420", False), ("p010", False), ("i010", False)):
        deep = fmt in K.YUV16
        shape = (K.T, h, w, 3) if fmt == "bgr24" else (K.T, h * 3 // 2, w)
        init = rs.randint(0, 65536 if deep else 256, shape[1:]).astype(np.uint16 if deep else np.uint8)
        for source in (True, False):
            got = PF.keep_borders_(torch.zeros(shape, dtype=torch.uint16 if deep else torch.uint8, device="cuda"), field, dev(init), fmt,
                                   initial_is_source=source, swap_rb=swap).cpu().numpy()
            want = init
            if source:
                want = init[..., ::-1] if swap else ((init >> 6) << 6 if fmt == "p010" else (np.minimum(init, 1023) if fmt == "i010" else init))
            assert all(np.array_equal(got[t], want) for t in range(K.T)), (fmt, swap, source)


def test_argument_checks(hip):
    from pwstablenet_amd import functional as PF
    A = hip
    lib, st = A.lib(), A.current_stream()
    EINVAL = -22
    field = torch.zeros((2, 4, 4, 2), device="cuda")
    u8 = torch.zeros(2 * 16 * 16 * 3, dtype=torch.uint8, device="cuda")
    u16 = torch.zeros(2 * 16 * 16 * 3, dtype=torch.uint16, device="cuda")
    p = A.ptr
    # (frames, field, initial, initial_is_source, n, h, w, fh, fw, swap_rb / layout, align_corners, bicubic, stream)
    assert lib.pws_border_keep_u8(p(u8), p(field), p(u8), 0, 2, 8, 8, 4, 4, 0, 0, 0, st) == 0
    assert lib.pws_border_keep_u8(p(u8), p(field), p(u8), 0, 2, 8, 6, 4, 4, 0, 0, 0, st) == EINVAL     # w % 4
    assert lib.pws_border_keep_u8(p(u8), p(field), p(u8), 0, 2, 8, 2, 4, 4, 0, 0, 0, st) == EINVAL     # w < 4
    assert lib.pws_border_keep_u8(p(u8), p(field), p(u8), 0, 2, 0, 8, 4, 4, 0, 0, 0, st) == EINVAL     # empty frame
    assert lib.pws_border_keep_u8(p(u8), p(field), p(u8), 0, 2, 8, 8, 0, 4, 0, 0, 0, st) == EINVAL     # empty field
    assert lib.pws_border_keep_u8(p(u8), p(field), None, 0, 2, 8, 8, 4, 4, 0, 0, 0, st) == EINVAL      # NULL initial
    assert lib.pws_border_keep_u8(p(u8[1:]), p(field), p(u8), 0, 2, 8, 8, 4, 4, 0, 0, 0, st) == EINVAL  # alignment
    for fn, buf in ((lib.pws_border_keep_yuv420_u8, u8), (lib.pws_border_keep_yuv420_u16, u16)):
        assert fn(p(buf), p(field), p(buf), 0, 2, 8, 8, 4, 4, 0, 0, 1, st) == 0
        assert fn(p(buf), p(field), p(buf), 0, 2, 7, 8, 4, 4, 0, 0, 0, st) == EINVAL    # odd h
        assert fn(p(buf), p(field), p(buf), 0, 2, 8, 6, 4, 4, 0, 0, 0, st) == EINVAL    # w % 4
        assert fn(p(buf), p(field), p(buf), 0, 2, 8, 4, 4, 4, 0, 0, 0, st) == 0         # w = 4: fine with the bilinear margin
        assert fn(p(buf), p(field), p(buf), 0, 2, 8, 4, 4, 4, 0, 0, 1, st) == EINVAL    # w >= 8 with the bicubic margin
        assert fn(p(buf), p(field), p(buf), 0, 2, 8, 8, 4, 4, 2, 0, 0, st) == EINVAL    # layout
        assert fn(p(buf), p(field), None, 0, 2, 8, 8, 4, 4, 0, 0, 0, st) == EINVAL      # NULL initial
    torch.cuda.synchronize()
    bgr = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):   # PWS_EINVAL through functional: w % 4
        PF.keep_borders_(torch.zeros((2, 8, 6, 3), dtype=torch.uint8, device="cuda"), field, torch.zeros((8, 6, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError):   # w >= 8 for 4:2:0 with the bicubic margin
        PF.keep_borders_(torch.zeros((2, 12, 4), dtype=torch.uint8, device="cuda"), field, torch.zeros((12, 4), dtype=torch.uint8, device="cuda"), "nv12",
                         mode="bicubic")
    with pytest.raises(ValueError):     # float frames: the feature is for the integer formats
        PF.keep_borders_(torch.zeros((2, 3, 8, 8), device="cuda"), field, torch.zeros((3, 8, 8), device="cuda"))
    with pytest.raises(ValueError):     # dtype / format mismatch, both ways
        PF.keep_borders_(torch.zeros((2, 12, 8), dtype=torch.uint8, device="cuda"), field, torch.zeros((12, 8), dtype=torch.uint8, device="cuda"), "p010")
    with pytest.raises(ValueError):
        PF.keep_borders_(torch.zeros((2, 12, 8), dtype=torch.uint16, device="cuda"), field, torch.zeros((12, 8), dtype=torch.uint16, device="cuda"), "nv12")
    with pytest.raises(ValueError):
        PF.keep_borders_(torch.zeros((2, 12, 8), dtype=torch.uint8, device="cuda"), field, torch.zeros((12, 8), dtype=torch.uint8, device="cuda"), "bgr24")
    with pytest.raises(ValueError):     # an unknown format or mode
        PF.keep_borders_(bgr, field, bgr[0], "yuv444")
    with pytest.raises(ValueError):
        PF.keep_borders_(bgr, field, bgr[0], mode="lanczos")
    with pytest.raises(ValueError):     # initial is one frame of the frames' layout; the field has one entry per frame
        PF.keep_borders_(bgr, field, bgr)
    with pytest.raises(ValueError):
        PF.keep_borders_(bgr, field[:1], bgr[0])
    with pytest.raises(RuntimeError):   # dtype of initial
        PF.keep_borders_(bgr, field, torch.zeros((8, 8, 3), dtype=torch.uint16, device="cuda"))
    assert PF.keep_borders_(bgr[:0], field[:0], torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")).shape[0] == 0   # an empty segment
