"""The float64 restatement of the bicubic warp (tests/bicubic_ref.py) against its oracle, torch-CPU float64 F.grid_sample(mode="bicubic"), and
the properties the definition promises; plus the argument check of the public ``mode`` switch.  No GPU."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bicubic_ref as B  # noqa: E402
import yuv16_ref as R16  # noqa: E402


@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("hw", [(9, 12), (38, 52)])
def test_restatement_equals_torch_float64(hw, ac):
    """Random bytes, coordinates out to +-1.5 (taps outside on every side), a field smaller than the plane: the restatement equals torch's
    bicubic grid_sample of the align_corners=True-resized field to 1e-9."""
    import torch.nn.functional as F
    h, w = hw
    rs = np.random.RandomState(h + ac)
    plane = rs.randint(0, 256, (2, h, w)).astype(np.float64)
    field = rs.uniform(-1.5, 1.5, (2, 5, 7, 2)).astype(np.float32)
    grid = R16._resize_field(field, h, w, np.float64)
    ref = F.grid_sample(torch.from_numpy(plane)[:, None], torch.from_numpy(grid), mode="bicubic", padding_mode="zeros", align_corners=ac)[:, 0]
    got = B.warp_plane(plane, field, ac, 0.0)
    err = float(np.abs(got - ref.numpy()).max())
    print("restatement vs torch float64 %s ac=%s: %.2e" % (hw, ac, err))
    assert err < 1e-9
    assert got.min() < 0 or got.max() > 255   # (the cubic leaves 0..255 on these inputs: the integer rule's clamp has work to do)


def test_weights_sum_to_one_and_pick_the_centre():
    t = np.linspace(0, 1, 1001)
    assert np.abs(np.sum(B.weights(t), 0) - 1).max() < 1e-14   # (a few float64 roundings of Horner terms of magnitude <= 4)
    assert B.weights(0.0) == [0.0, 1.0, 0.0, 0.0]
    # t = 0 everywhere: a field at the plane's own power-of-two size, align_corners=False -> the plane itself, exactly
    plane = np.random.RandomState(0).randint(0, 256, (1, 8, 16)).astype(np.float64)
    assert np.array_equal(B.warp_plane(plane, B.affine_field(1, 8, 16), False, 16.0), plane)


@pytest.mark.parametrize("pad", [0.0, 16.0, 128.0, 64.0, 512.0])
def test_all_outside_is_pad_exactly(pad):
    plane = np.random.RandomState(1).randint(0, 1024, (2, 6, 8)).astype(np.float64)
    for shift in (3e4, -3e4):
        field = B.affine_field(2, 5, 7, shift=(shift, -shift))
        assert B.all_outside(field, 6, 8, False).all()
        assert np.array_equal(B.warp_plane(plane, field, False, pad), np.full(plane.shape, pad))
    # a zoom-out: the all-outside pixels are pad exactly, the others are not all pad
    field = B.affine_field(2, 5, 7, scale=1.3, shift=(0.9, 0.8))
    out, fl = B.all_outside(field, 6, 8, False), B.warp_plane(plane, field, False, pad)
    assert 0.05 < out.mean() < 0.95 and (fl[out] == pad).all() and (fl[~out] != pad).any()


def test_integer_rule_clamps_overshoot_and_undershoot():
    """Half way between the two middle columns of (0, hi, hi, 0) the cubic gives 1.1875 hi, of (hi, 0, 0, hi) -0.1875 hi: the integer rule
    clamps them to hi and to 0 (8 and 10 bits); float output keeps them."""
    for hi in (255, 1023):
        over = np.tile(np.array([0, hi, hi, 0], np.float64), (1, 4, 1))
        # a constant field: every output sample reads (ix, iy) = (1.5, 1.5) (align_corners=False, w = h = 4: g = 0)
        field = np.zeros((1, 2, 2, 2), np.float32)
        fo, fu = B.warp_plane(over, field, False, 0.0), B.warp_plane(hi - over, field, False, 0.0)
        assert np.allclose(fo, 1.1875 * hi) and np.allclose(fu, -0.1875 * hi)
        assert (B.quantize(fo, hi) == hi).all() and (B.quantize(fu, hi) == 0).all()
    assert (B.quantize(np.array([254.999, 255.0, 17.0, 17.9999]), 255) == [254, 255, 17, 17]).all()
    u8, fl = B.warp_bgr(np.tile(np.array([0, 255, 255, 0], np.uint8)[None, None, :, None], (1, 4, 1, 3)), np.zeros((1, 2, 2, 2), np.float32))
    assert (u8 == 255).all() and fl.max() > 300


def test_packed_formats_use_their_own_pad_and_placement():
    """Everything outside: Y is black, chroma is grey, in every format's placement; junk in P010's low bits does not reach the output."""
    field = B.affine_field(1, 5, 7, shift=(3e4, 3e4))
    for fmt in ("nv12", "i420"):
        f = np.random.RandomState(2).randint(0, 256, (1, 12, 8)).astype(np.uint8)
        got, fl = B.warp_yuv(f, field, fmt)
        assert got.dtype == np.uint8 and (got[:, :8] == 16).all() and (got[:, 8:] == 128).all() and np.array_equal(fl, got)
    for fmt in ("p010", "i010"):
        f = np.random.RandomState(3).randint(0, 65536, (1, 12, 8)).astype(np.uint16)
        got, fl = B.warp_yuv16(f, field, fmt)
        assert got.dtype == np.uint16 and (R16.samples(got[:, :8], fmt) == 64).all() and (R16.samples(got[:, 8:], fmt) == 512).all()
        if fmt == "p010":
            assert (got & 63 == 0).all()


def test_unknown_mode_is_a_value_error_before_the_library():
    """``mode`` is checked first: no device tensor, no library needed.  (The parent of this change has no ``mode`` argument.)"""
    from pwstablenet_amd import functional as PF
    u8, field = torch.zeros((1, 8, 8, 3), dtype=torch.uint8), torch.zeros((1, 4, 4, 2))
    with pytest.raises(ValueError):
        PF.upsample_grid_sample_u8(u8, field, mode="lanczos")
    with pytest.raises(ValueError):
        PF.upsample_grid_sample(torch.zeros((1, 3, 8, 8)), field, mode="nearest")
    with pytest.raises(ValueError):
        PF.upsample_grid_sample_yuv420(torch.zeros((1, 12, 8), dtype=torch.uint8), field, "nv12", mode="lanczos")
    with pytest.raises(ValueError):
        PF.upsample_grid_sample_yuv420_16(torch.zeros((1, 12, 8), dtype=torch.uint16), field, "p010", mode="lanczos")
    from pwstablenet_amd.stream import VideoStabilizer
    with pytest.raises(ValueError):
        VideoStabilizer(torch.nn.Identity(), device="cpu", interpolation="lanczos")
    assert VideoStabilizer(torch.nn.Identity(), device="cpu").interpolation == "bilinear"
