"""CPU tests of the numpy restatement of the 10-bit 4:2:0 path (tests/yuv16_ref.py): they pin it to the 8-bit restatement
(tests/yuv_ref.py) wherever the two must agree, check the packing, the reduction and the black padding, and measure what fp32 arithmetic
costs against float64 on the inputs the GPU warp tests use (which makes their tolerance meaningful)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv16_ref as R16  # noqa: E402
import yuv_ref as R  # noqa: E402

FMTS = ["p010", "i010"]
WARP_SHAPES = R16.WARP_SHAPES


@pytest.mark.parametrize("fmt", FMTS)
def test_pack_unpack_round_trip(fmt):
    rs = np.random.RandomState(1)
    y, u, v = rs.randint(0, 1024, (2, 8, 12)), rs.randint(0, 1024, (2, 4, 6)), rs.randint(0, 1024, (2, 4, 6))
    f = R16.pack(y, u, v, fmt)
    assert f.dtype == np.uint16 and f.shape == (2, 12, 12)
    for a, b in zip(R16.unpack(f, fmt), (y, u, v)):
        assert np.array_equal(a, b)
    assert np.array_equal(R16.pack(*R16.unpack(f, fmt), fmt), f)
    if fmt == "p010":
        assert (f & 63 == 0).all() and np.array_equal(f[:, :8] >> 6, y)
        assert np.array_equal(f[:, 8:, 0::2] >> 6, u) and np.array_equal(f[:, 8:, 1::2] >> 6, v)
    else:
        assert np.array_equal(f[:, :8], y) and np.array_equal(f[:, 8:].reshape(2, 2, 4, 6)[:, 1], v)


def test_reduction():
    v8 = np.arange(256)
    assert np.array_equal(R16.reduce8(v8 << 2), v8)
    assert R16.reduce8(1023) == 255 and R16.reduce8(1022) == 255 and R16.reduce8(1021) == 255 and R16.reduce8(1017) == 254
    assert R16.reduce8(1) == 0 and R16.reduce8(2) == 1 and R16.reduce8(5) == 1 and R16.reduce8(6) == 2   # round to nearest, half up
    for fmt in FMTS:
        f8 = R.random_yuv(1, 8, 8, R16.FMT8[fmt], seed=4, smooth=False)
        assert np.array_equal(R16.reduce(R16.expand(f8, fmt), fmt), f8)


def test_p010_low_bits_are_ignored_and_i010_clamps():
    rs = np.random.RandomState(2)
    f = R16.random_yuv16(1, 8, 8, "p010", seed=2)
    junk = (f | rs.randint(0, 64, f.shape).astype(np.uint16)).astype(np.uint16)
    assert (junk != f).any()
    assert np.array_equal(R16.samples(junk, "p010"), R16.samples(f, "p010"))
    assert np.array_equal(R16.reduce(junk, "p010"), R16.reduce(f, "p010"))
    field = R16.smooth_field(1, 3, size=16)
    assert np.array_equal(R16.warp_yuv(junk, field, "p010"), R16.warp_yuv(f, field, "p010"))
    assert np.array_equal(R16.area_resize_yuv16(junk, "p010", (4, 4)), R16.area_resize_yuv16(f, "p010", (4, 4)))
    assert R16.samples(np.array([1023, 1024, 65535], np.uint16), "i010").tolist() == [1023, 1023, 1023]


@pytest.mark.parametrize("fmt", FMTS)
def test_window_planes_of_expanded_frames_equal_the_8bit_planes(fmt):
    f8 = R.random_yuv(2, 48, 64, R16.FMT8[fmt], seed=5)
    assert np.array_equal(R16.window_planes(R16.expand(f8, fmt), fmt, 24), R.window_planes(f8, R16.FMT8[fmt], 24))
    f16 = R16.random_yuv16(1, 48, 64, fmt, seed=6, smooth=False)   # any words: the planes of the reduced clip
    assert np.array_equal(R16.window_planes(f16, fmt, 24), R.window_planes(R16.reduce(f16, fmt), R16.FMT8[fmt], 24))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [(32, 24), (16, 12), (20, 14)])   # from 64 x 48: 2 x 2, integer (4 x 4; chroma too), fractional
def test_area_resize_of_8bit_values_equals_the_8bit_restatement(fmt, size):
    f8 = R.random_yuv(2, 48, 64, R16.FMT8[fmt], seed=size[0], smooth=False)
    as16 = R16.place(f8, fmt)   # the same numbers (<= 255) as 10-bit samples
    got = R16.area_resize_yuv16(as16, fmt, size)
    assert np.array_equal(R16.samples(got, fmt), R.area_resize_yuv(f8, R16.FMT8[fmt], size).astype(np.int64))
    if fmt == "p010":
        assert (got & 63 == 0).all()


@pytest.mark.parametrize("fmt", FMTS)
def test_area_resize_keeps_ten_bits(fmt):
    """A constant 1023 stays 1023 in every branch (no 8-bit clamp anywhere), and a 2 x 2 block rounds half up."""
    f = R16.pack(np.full((1, 48, 64), 1023), np.full((1, 24, 32), 1000), np.full((1, 24, 32), 900), fmt)
    for size in [(32, 24), (16, 12), (20, 14)]:
        y, u, v = R16.unpack(R16.area_resize_yuv16(f, fmt, size), fmt)
        assert (y == 1023).all() and (u == 1000).all() and (v == 900).all()
    blk = R16.resize_area_u10(np.array([[[1000], [1001]], [[1001], [1000]]]), 1, 1)
    assert blk[0, 0, 0] == 1001   # (4002 + 2) >> 2


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("ac", [False, True])
def test_whole_pixel_translation_shifts_samples_and_pads_black(fmt, ac):
    """A field that moves a plane by whole pixels reproduces the shifted samples exactly and reads black, 64 in Y and 512 in U and V, where
    the source falls outside.  Every plane is warped by the field resized to the plane's OWN size, so a field given at the luma plane's size
    is a whole-pixel translation for Y, and one given at the chroma planes' size is one for U and V."""
    t, h, w = 2, 16, 32
    f = R16.random_yuv16(t, h, w, fmt, seed=9, smooth=False)
    planes = dict(zip("yuv", R16.unpack(f, fmt)))
    dx, dy = 3, 2   # output (y, x) reads source (y + dy, x + dx)

    def translation(ph, pw):
        if ac:
            gx, gy = (np.arange(pw) + dx) / (pw - 1) * 2 - 1, (np.arange(ph) + dy) / (ph - 1) * 2 - 1
        else:
            gx, gy = (2 * (np.arange(pw) + dx) + 1) / pw - 1, (2 * (np.arange(ph) + dy) + 1) / ph - 1
        return np.broadcast_to(np.stack(np.meshgrid(gx, gy, indexing="xy"), -1), (t, ph, pw, 2)).copy()
    for names, (ph, pw), pad in (("y", (h, w), 64), ("uv", (h // 2, w // 2), 512)):
        words = R16.warp_yuv(f, translation(ph, pw), fmt, ac)
        out = dict(zip("yuv", R16.unpack(words, fmt)))
        for k in names:
            want = np.full_like(planes[k], pad)
            want[:, :ph - dy, :pw - dx] = planes[k][:, dy:, dx:]
            # (float64 coordinates land within 1e-12 of the integer, the blend within 1e-9 of the sample: the truncation absorbs that)
            assert np.array_equal(out[k], want), (fmt, ac, k)
        if fmt == "p010":
            assert (words & 63 == 0).all()


def test_padding_is_bt601_black_at_ten_bits():
    f = R16.random_yuv16(1, 8, 8, "p010", seed=2)
    far = np.full((1, 4, 4, 2), 5.0)   # every tap far outside the frame
    out = R16.warp_yuv(f, far, "p010")
    y, u, v = R16.unpack(out, "p010")
    assert (y == 64).all() and (u == 512).all() and (v == 512).all()
    assert (out[:, :8] == 64 << 6).all() and (out[:, 8:] == 512 << 6).all()
    assert (R.yuv2bgr(R16.reduce(out, "p010"), "nv12") == 0).all()   # black is black after the reduction too (16, 128, 128)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("shape", WARP_SHAPES + ["border"])
def test_float32_restatement_meets_the_gpu_tests_acceptance(fmt, ac, shape):
    """What makes the GPU warp tests' tolerance meaningful: the restatement evaluated in float32 (every operation rounded to fp32, as a
    kernel's are, in one particular order) on the very inputs tests/test_hip_yuv16.py uses (yuv16_ref.warp_case / border_case) must itself
    pass the acceptance function those tests apply against the float64 restatement -- at most 1 LSB of 10 bits off, only where the
    float64 blend lies within 0.05 of an integer, below the 8-bit test's cap of 6e-2 of the samples.  warp_case's docstring says how the
    inputs were chosen for that.
    Measured float32 shares of differing samples (either format): 720 x 1280 1.6e-4, 90 x 896 1.2e-4 to 1.7e-4, 48 x 64 and 38 x 52 at most
    6.8e-4, the border case 4.9e-3 (align_corners False) / 6.4e-3 (True): an order of magnitude or more under the cap."""
    f, field = R16.border_case(fmt) if shape == "border" else R16.warp_case(shape, fmt)
    ref, ref_f = R16.warp_yuv(f, field, fmt, ac, return_float=True)
    got32 = R16.warp_yuv(f, field, fmt, ac, dtype=np.float32)
    share = R16.accept(got32, ref, ref_f, fmt)
    print("float32 share of differing samples %s ac=%s %s: %.2e" % (fmt, ac, shape, share))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("ac", [False, True])
def test_float32_restatement_meets_the_wide_border_acceptance(fmt, ac):
    """The same for the 720p case whose field zooms out (yuv16_ref.wide_border_case, judged by accept_wide): the float32 restatement is at
    most 1 LSB off everywhere and inside the 0.05 band wherever all four taps are inside a plane, and the case is not vacuous: more than
    1 % of the samples read black only, and some straddle an edge of a wide plane.  (Exact black where all taps are outside is part of the
    definition, not a property of fp32 arithmetic -- see accept_wide -- so it is asked of the kernel only.)
    Measured float32 shares of differing samples (either format): 3.6e-4 (align_corners False) / 3.8e-4 (True), with 1.9e-3 / 1.8e-3 of
    the samples straddling an edge and 1.9 % / 1.8 % reading black only."""
    f, field = R16.wide_border_case(fmt)
    ref, ref_f = R16.warp_yuv(f, field, fmt, ac, return_float=True)
    inside, outside = R16.tap_masks(f.shape, field, fmt, ac)
    assert not (inside & outside).any() and outside.mean() > 0.01 and (~inside & ~outside).mean() > 1e-3
    got32 = R16.warp_yuv(f, field, fmt, ac, dtype=np.float32)
    share, straddle = R16.accept_wide(got32, ref, ref_f, fmt, inside, outside, exact_black=False)
    print("float32 share of differing samples %s ac=%s wide border: %.2e (straddling an edge: %.2e, black only: %.2e)"
          % (fmt, ac, share, straddle, outside.mean()))
