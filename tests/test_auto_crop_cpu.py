"""CPU half of the automatic crop (reference main_new.py:484-606): the float64 restatement of the fit (tests/homography_ref.py)
recovers exact correspondences, and the host recurrence ``stream.auto_crop_window`` against hand-computed windows."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_ref as R  # noqa: E402

from pwstablenet_amd.stream import auto_crop_window  # noqa: E402


def _apply(M, p):
    q = p @ M[:2, :2].T + M[:2, 2]
    return q / (p @ M[2, :2] + M[2, 2])[:, None]


@pytest.mark.parametrize("frame_hw", [(360, 640), (720, 1280)])
@pytest.mark.parametrize("kind", ["affine", "projective"])
def test_restatement_recovers_exact_correspondences(frame_hw, kind):
    _, _, p2 = R.lattice(frame_hw)
    M = np.array([[0.93, 0.04, 0.02], [-0.03, 1.06, -0.015], [0.0, 0.0, 1.0]])
    if kind == "projective":
        M[2, :2] = (0.05, -0.03)
    p1 = _apply(np.linalg.inv(M), p2)          # p2 = M(p1) exactly (in float64)
    got = R.fit(p1, p2)
    assert got is not None
    assert np.abs(got - M).max() < 1e-12, np.abs(got - M).max()


def test_restatement_lattice_and_degenerate_samples():
    r, c, p2 = R.lattice((360, 640))
    assert (r.min(), r.max(), c.min(), c.max()) == (30, 315, 20, 590)
    assert p2[0, 0] == np.float32((320 - 300) / 640 * 2 - 1) and p2[21, 1] == np.float32(45 / 360 * 2 - 1)
    assert R.fit(np.full((400, 2), 0.25), p2) is None                   # a constant field has no homography
    assert np.all(np.isnan(R.bounds(None, (360, 640))))
    b = R.bounds(np.eye(3), (360, 640))                                  # identity: the corners themselves
    assert b[0] == 0 and b[2] == 0 and b[1] == pytest.approx((R.CORNER + 1) * 180) and b[3] == pytest.approx((R.CORNER + 1) * 320)


def test_constant_bounds_halve_the_gap_per_updated_frame():
    period, T = 30, 40
    top, bottom, left, right = 20.0, 340.0, 40.0, 600.0
    got = auto_crop_window([[top, bottom, left, right]] * T, (360, 640), period=period)
    k = len([i for i in range(T) if 15 < i < T - 15])                    # frames 16 .. 24
    assert k == 9
    f = 1 - 0.5 ** k
    want = (left * f, 640 - (640 - right) * f, top * f, 360 - (360 - bottom) * f)
    assert got == pytest.approx(want, rel=0, abs=1e-12)
    assert got == pytest.approx(R.crop_window(np.array([[top, bottom, left, right]] * T), (360, 640)), abs=1e-12)


@pytest.mark.parametrize("T", [0, 1, 16, 31])
def test_no_update_for_short_clips(T):
    # the recurrence needs a frame with 15 < i < T - 15: none for T <= period + 1
    assert auto_crop_window([[50.0, 300.0, 60.0, 500.0]] * T, (360, 640), period=30) == (0.0, 640.0, 0.0, 360.0)
    assert auto_crop_window([[50.0, 300.0, 60.0, 500.0]] * 32, (360, 640), period=30) == (30.0, 570.0, 25.0, 330.0)


def test_first_and_last_half_period_are_ignored():
    T, half = 40, 15
    bnds = np.tile([[0.0, 360.0, 0.0, 640.0]], (T, 1))
    bnds[:half + 1] = [100.0, 200.0, 100.0, 200.0]                       # frames 0 .. 15: not read
    bnds[T - half:] = [100.0, 200.0, 100.0, 200.0]                       # frames 25 .. 39: not read
    assert auto_crop_window(bnds, (360, 640)) == (0.0, 640.0, 0.0, 360.0)
    bnds[half + 1] = [10.0, 350.0, 20.0, 630.0]                          # the first frame that is read
    assert auto_crop_window(bnds, (360, 640)) == (10.0, 635.0, 5.0, 355.0)
    bnds[half + 1] = [0.0, 360.0, 0.0, 640.0]
    bnds[T - half - 1] = [10.0, 350.0, 20.0, 630.0]                      # the last one
    assert auto_crop_window(bnds, (360, 640)) == (10.0, 635.0, 5.0, 355.0)


def test_edges_move_only_outwards_of_the_bounds():
    bnds = np.tile([[0.0, 360.0, 0.0, 640.0]], (33, 1))
    bnds[16] = [-30.0, 400.0, -5.0, 700.0]                                # bounds outside the frame pull nothing
    bnds[17] = [8.0, 352.0, 16.0, 624.0]
    assert auto_crop_window(bnds, (360, 640)) == (8.0, 632.0, 4.0, 356.0)


def test_nan_bounds_only_matter_in_frames_that_are_read():
    T = 40
    bnds = np.tile([[10.0, 350.0, 20.0, 620.0]], (T, 1))
    bnds[3] = np.nan
    bnds[T - 2] = np.nan
    auto_crop_window(bnds, (360, 640))                                     # ignored frames: accepted
    bnds[20, 2] = np.nan
    with pytest.raises(ValueError, match="frame 20"):
        auto_crop_window(bnds, (360, 640))
    import torch
    with pytest.raises(ValueError, match="frame 20"):
        auto_crop_window(torch.from_numpy(bnds.astype(np.float32)), (360, 640))


def test_empty_window_raises():
    bnds = np.tile([[200.0, 100.0, 20.0, 620.0]], (40, 1))               # top below bottom: the window closes
    with pytest.raises(ValueError, match="empty"):
        auto_crop_window(bnds, (360, 640))
    bnds = np.tile([[10.0, 350.0, 400.0, 200.0]], (40, 1))
    with pytest.raises(ValueError, match="empty"):
        auto_crop_window(bnds, (360, 640))


def test_output_size_scaling():
    bnds = np.tile([[20.0, 340.0, 40.0, 600.0]], (32, 1))                 # one updated frame of a 1280 x 720 source
    assert auto_crop_window(bnds, (720, 1280)) == (20.0, 940.0, 10.0, 530.0)
    assert auto_crop_window(bnds, (720, 1280), output_hw=(360, 640)) == (10.0, 470.0, 5.0, 265.0)
    x0, x1, y0, y1 = auto_crop_window(bnds, (720, 1280), output_hw=(300, 500))
    assert (x0, x1, y0, y1) == pytest.approx((20 * 500 / 1280, 940 * 500 / 1280, 10 * 300 / 720, 530 * 300 / 720), abs=1e-12)
    assert math.isclose(x1, 367.1875)
