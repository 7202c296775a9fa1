"""CPU tests of zoom to fill: the float64 restatement tests/zoom_ref.py against the analytic composition on affine fields, and the host
arithmetic of pwstablenet_amd.stream.zoom_window / zoom_schedule and functional.zoom_coefficients."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zoom_ref as Z  # noqa: E402

from pwstablenet_amd import functional as PF  # noqa: E402
from pwstablenet_amd.stream import zoom_schedule, zoom_window  # noqa: E402

FRAME = (360, 640)
WINDOWS = {"whole": (0.0, 640.0, 0.0, 360.0), "half": (160.0, 480.0, 90.0, 270.0), "partial": (0.0, 512.5, 0.0, 300.25),
           "off-centre": (101.3, 620.9, 33.7, 341.2)}


@pytest.mark.parametrize("name", list(WINDOWS))
@pytest.mark.parametrize("field_hw", [(256, 256), (24, 40), (2, 2)])
def test_restatement_is_the_analytic_composition_on_affine_fields(name, field_hw):
    """G(px, py) = a + b px + c py over the frame's pixel coordinates, sampled at the field's nodes (node j = pixel j (W0-1)/(fw-1)).  The
    bilinear interpolation of an affine function is exact, so the zoomed field's node must hold G at the pixel coordinate the definition
    gives it: the centre of output pixel x mapped into the window, x0 + (x + 0.5) (x1 - x0) / W0 - 0.5, clamped to the frame."""
    h0, w0 = FRAME
    fh, fw = field_hw
    x0, x1, y0, y1 = WINDOWS[name]
    px, py = np.arange(fw) * (w0 - 1) / (fw - 1), np.arange(fh) * (h0 - 1) / (fh - 1)
    coefs = [(0.3, 1.1e-3, -0.4e-3), (-0.2, 0.2e-3, 1.7e-3)]
    G = lambda c, X, Y: c[0] + c[1] * X + c[2] * Y   # noqa: E731
    field = np.stack([G(c, px[None, :], py[:, None]) for c in coefs], -1)[None]
    got = Z.zoom64(field, Z.coefficients([WINDOWS[name]], FRAME, field_hw))
    qx = np.clip(x0 + (px + 0.5) * (x1 - x0) / w0 - 0.5, 0, w0 - 1)
    qy = np.clip(y0 + (py + 0.5) * (y1 - y0) / h0 - 0.5, 0, h0 - 1)
    want = np.stack([G(c, qx[None, :], qy[:, None]) for c in coefs], -1)[None]
    err = np.abs(got - want).max()
    print("%s %s: largest error %.3g" % (name, field_hw, err))
    assert err <= 1e-12


def test_whole_frame_is_the_identity():
    c = Z.coefficients([WINDOWS["whole"]], FRAME, (256, 256))
    assert np.array_equal(c, [[0.0, 1.0, 0.0, 1.0]])
    field = Z.make_field((2, 67, 129, 2), 1)
    c = Z.coefficients([WINDOWS["whole"]] * 2, FRAME, (67, 129))
    assert np.array_equal(Z.zoom64(field, c), field.astype(np.float64))
    assert np.array_equal(Z.zoom32(field, c), field)
    # the package's own coefficients: float64 on the host, rounded once
    mine = PF.zoom_coefficients(PF._zoom_windows(WINDOWS["whole"], 2, FRAME), FRAME, (67, 129)).numpy()
    assert mine.dtype == np.float32 and np.array_equal(mine, c)
    wins = list(WINDOWS.values())
    mine = PF.zoom_coefficients(PF._zoom_windows(wins, 4, FRAME), FRAME, (256, 256)).numpy()
    assert np.array_equal(mine, Z.coefficients(wins, FRAME, (256, 256)).astype(np.float32))


def test_windows_outside_the_frame_are_refused():
    for bad in [(-0.1, 640, 0, 360), (0, 640.5, 0, 360), (0, 640, 10, 10), (300, 200, 0, 360), (0, 640, 0, float("nan")), (0, 640, 0)]:
        with pytest.raises(ValueError):
            PF._zoom_windows(bad, 1, FRAME)
    with pytest.raises(ValueError):
        PF._zoom_windows([WINDOWS["whole"]] * 3, 2, FRAME)


@pytest.mark.parametrize("window", [(0.0, 640.0, 0.0, 360.0), (17.45, 602.1, 20.9, 347.4), (100.0, 200.0, 10.0, 350.0), (0.0, 333.3, 0.0, 360.0)])
def test_zoom_window_has_the_frame_aspect_lies_inside_and_is_maximal(window):
    h0, w0 = FRAME
    x0, x1, y0, y1 = zoom_window(window, FRAME)
    assert window[0] <= x0 < x1 <= window[1] and window[2] <= y0 < y1 <= window[3]
    assert abs((x1 - x0) / w0 - (y1 - y0) / h0) <= 1e-12                                       # the frame's aspect
    assert abs((x0 + x1) - (window[0] + window[1])) <= 1e-9 and abs((y0 + y1) - (window[2] + window[3])) <= 1e-9   # centred
    # maximal: it spans its argument along one axis
    assert min(window[1] - window[0] - (x1 - x0), window[3] - window[2] - (y1 - y0)) <= 1e-9
    if window == (0.0, 640.0, 0.0, 360.0):
        assert (x0, x1, y0, y1) == window


def _k_of(windows, frame_hw):
    h0, w0 = frame_hw
    w = np.asarray(windows, np.float64)
    k = (w[:, 1] - w[:, 0]) / w0
    assert np.abs((w[:, 3] - w[:, 2]) / h0 - k).max() <= 1e-12                                   # the frame's aspect
    assert np.abs(w[:, 0] + w[:, 1] - w0).max() <= 1e-9 and np.abs(w[:, 2] + w[:, 3] - h0).max() <= 1e-9   # the frame's centre
    return k


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_zoom_schedule_is_the_envelope(seed):
    h0, w0 = FRAME
    T, cut, speed, kmin = 70, 31, 0.004, 0.6
    rs = np.random.RandomState(seed)
    # per frame: bounds outside the frame (asks for no zoom), a small wedge, or a wedge that asks for more than 1 / kmin
    lo, hi = np.array([[-5.0, 0.0], [0.0, 0.12], [0.15, 0.3]])[rs.randint(0, 3, T)].T
    draw = lambda size: np.where(lo < 0, rs.uniform(-5, 0, T), rs.uniform(lo, hi) * size)   # noqa: E731
    top, left = draw(h0), draw(w0)
    bottom, right = h0 - draw(h0), w0 - draw(w0)
    bounds = np.stack([top, bottom, left, right], 1)
    k_req = np.minimum(1.0, np.minimum(2 * np.minimum(w0 / 2 - left, right - w0 / 2) / w0, 2 * np.minimum(h0 / 2 - top, bottom - h0 / 2) / h0))
    kc = np.maximum(k_req, kmin)
    assert (k_req < kmin).any() and (k_req == 1.0).any() and ((k_req > kmin) & (k_req < 1)).any()   # every branch of the rule is drawn
    k = _k_of(zoom_schedule(bounds, FRAME, speed, kmin, scene_cuts=[cut]), FRAME)
    want = np.empty(T)
    for a, b in ((0, cut), (cut, T)):   # the O(T^2) envelope, scene by scene
        for t in range(a, b):
            want[t] = min(kc[s] + speed * abs(t - s) for s in range(a, b))
    assert np.abs(k - want).max() <= 1e-12
    assert (k <= kc + 1e-12).all()
    d = np.abs(np.diff(k))
    inside = np.ones(T - 1, bool)
    inside[cut - 1] = False
    assert (d[inside] <= speed + 1e-12).all()
    # free across a cut: without it the two scenes constrain each other
    one = _k_of(zoom_schedule(bounds, FRAME, speed, kmin), FRAME)
    assert (one <= k + 1e-12).all()
    kc2 = kc.copy()
    kc2[:cut], kc2[cut:] = 1.0, kmin
    b2 = np.stack([np.where(kc2 == 1.0, 0.0, h0 / 2 * (1 - kmin)), np.where(kc2 == 1.0, h0, h0 / 2 * (1 + kmin)), np.zeros(T), np.full(T, w0)], 1)
    jump = _k_of(zoom_schedule(b2, FRAME, speed, kmin, scene_cuts=[cut]), FRAME)
    assert np.abs(jump[:cut] - 1.0).max() <= 1e-12 and np.abs(jump[cut:] - kmin).max() <= 1e-12
    # accepts a tensor as field_homography returns it
    import torch
    assert np.abs(_k_of(zoom_schedule(torch.from_numpy(bounds), FRAME, speed, kmin, scene_cuts=[cut]), FRAME) - k).max() == 0


def test_zoom_schedule_refuses_nan_bounds():
    bounds = [[0.0, 360.0, 0.0, 640.0]] * 5
    bounds[3] = [0.0, float("nan"), 0.0, 640.0]
    with pytest.raises(ValueError, match="frame 3"):
        zoom_schedule(bounds, FRAME)
    with pytest.raises(ValueError):
        zoom_schedule([[0.0, 360.0, 0.0]], FRAME)


def test_float32_sequence_is_close_and_the_undecided_share_is_small():
    """The yardstick of tests/test_hip_zoom.py, on its fields: prints the float32 restatement's error and the share of nodes within delta of a
    coverage threshold (the GPU test asserts the cap on the reference alone, before it looks at the kernel)."""
    C = Z
    for shape in C.SHAPES:
        field = Z.make_field(shape, C.seed_of(shape))
        for wins in C.window_rounds(shape):
            coef = Z.coefficients(wins, C.FRAME, shape[1:3])
            e32 = np.abs(Z.zoom32(field, coef).astype(np.float64) - Z.zoom64(field, coef)).max()
            assert e32 <= 16 * np.finfo(np.float32).eps * np.abs(field).max()
        field = Z.make_field(shape, C.seed_of(shape), scale=C.COVER_SCALE)
        for ac in (False, True):
            for m in (0, 1):
                lo, hi, share, delta = Z.count_bounds(field, Z.coefficients(C.window_rounds(shape)[0], C.FRAME, shape[1:3]), C.FRAME, ac, m)
                print("%s ac=%s m=%d: uncovered %s .. %s, undecided share %.4f, delta %.3g px, fp32 error %.3g" % (shape, ac, m, lo, hi, share, delta, e32))
                assert share <= Z.CAP
