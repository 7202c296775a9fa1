"""CPU test of the numpy restatement of the 4:2:0 YUV path (tests/yuv_ref.py): the BT.601 conversion at known colours, the warp's
identity and black padding, and the equivalence of the NV12 and I420 packings."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref as R  # noqa: E402


def solid(y, u, v, fmt, h=4, w=8):
    return R.pack(np.full((1, h, w), y, np.uint8), np.full((1, h // 2, w // 2), u, np.uint8), np.full((1, h // 2, w // 2), v, np.uint8), fmt)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_bt601_black_white_and_colours(fmt):
    assert (R.yuv2bgr(solid(16, 128, 128, fmt), fmt) == 0).all()
    assert (R.yuv2bgr(solid(235, 128, 128, fmt), fmt) == 255).all()
    assert (R.yuv2bgr(solid(0, 128, 128, fmt), fmt) == 0).all()        # below black clamps at 0
    # hand-computed from the fixed point: y = (Y - 16) * 1220542, B = (y + 2116026 u + 2^19) >> 20, ...
    for (y, u, v), bgr in [((81, 90, 240), (0, 0, 255)),     # BT.601 red
                           ((145, 54, 34), (0, 255, 0)),      # green
                           ((41, 240, 110), (255, 0, 0)),     # blue
                           ((126, 128, 128), (128, 128, 128)),
                           ((100, 150, 90), (142, 120, 37))]:
        got = tuple(int(c) for c in R.yuv2bgr(solid(y, u, v, fmt), fmt)[0, 0, 0])
        yy, uu, vv = (y - 16) * 1220542, u - 128, v - 128
        want = tuple(min(255, max(0, (yy + k + (1 << 19)) >> 20)) for k in (2116026 * uu, -852492 * vv - 409993 * uu, 1673527 * vv))
        assert got == want
        assert max(abs(a - b) for a, b in zip(got, bgr)) <= 1, (y, u, v, got, bgr)


def test_chroma_is_taken_from_the_2x2_block_without_interpolation():
    f = R.random_yuv(1, 6, 8, "i420", seed=1, smooth=False)
    y, u, v = R.unpack(f, "i420")
    bgr = R.yuv2bgr(f, "i420")
    for yy in range(6):
        for xx in range(8):
            one = R.pack(y[:, yy:yy + 2, xx:xx + 2][:, :1, :1].repeat(2, 1).repeat(2, 2), u[:, yy // 2:yy // 2 + 1, xx // 2:xx // 2 + 1],
                         v[:, yy // 2:yy // 2 + 1, xx // 2:xx // 2 + 1], "i420")
            assert (R.yuv2bgr(one, "i420")[0, 0, 0] == bgr[0, yy, xx]).all()


def identity_field(t, n=256):
    """The align_corners=True identity: resized to any plane size it maps every pixel onto itself."""
    g = np.linspace(-1, 1, n)
    return np.broadcast_to(np.stack(np.meshgrid(g, g, indexing="xy"), -1), (t, n, n, 2)).copy()


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_identity_field_returns_the_input(fmt):
    f = R.random_yuv(2, 24, 32, fmt, seed=3, smooth=False)
    assert np.array_equal(R.warp_yuv(f, identity_field(2), fmt, align_corners=True), f)


def test_nv12_and_i420_packings_give_the_same_planes():
    f = R.random_yuv(2, 36, 48, "i420", seed=5)
    y, u, v = R.unpack(f, "i420")
    g = R.pack(y, u, v, "nv12")
    assert np.array_equal(R.yuv2bgr(f, "i420"), R.yuv2bgr(g, "nv12"))
    rs = np.random.RandomState(0)
    field = identity_field(2, 16) * 1.1 + 0.05 * rs.standard_normal((2, 16, 16, 2))
    same = lambda a, b: all(np.array_equal(p, q) for p, q in zip(R.unpack(a, "i420"), R.unpack(b, "nv12")))   # noqa: E731
    for ac in (False, True):
        assert same(R.warp_yuv(f, field, "i420", ac), R.warp_yuv(g, field, "nv12", ac))
    assert same(R.area_resize_yuv(f, "i420", (20, 14)), R.area_resize_yuv(g, "nv12", (20, 14)))


def test_padding_is_bt601_black():
    f = R.random_yuv(1, 8, 8, "nv12", seed=2)
    far = np.full((1, 4, 4, 2), 5.0)   # every tap far outside the frame
    out = R.warp_yuv(f, far, "nv12")
    y, u, v = R.unpack(out, "nv12")
    assert (y == 16).all() and (u == 128).all() and (v == 128).all()
    assert (R.yuv2bgr(out, "nv12") == 0).all()
