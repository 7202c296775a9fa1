"""CPU tests of the float64 restatement of rolling-shutter correction (tests/shutter_ref.py): the definitions' own fixed points, and the
analytic experiment that motivates the feature -- a camera with a known continuous path and a rolling shutter, its frames smoothed with
and without the row-dependent correction, and how far from rigid the output frames are.

The experiment's parameters (shutter_ref: N = 32 frames of 256 x 256, r = 0.8, sigma = 4, a 33 x 33 lattice; a pan of (1.5, 0.5) pixels a
frame, shake of 3 and 1.5 pixels with periods of 13 and 29 frames in x, 2.5 and 1 pixel with 17 and 11 frames in y, 0.2 degree with 19
frames) were chosen before any kernel existed, with the float64 restatement alone: e(+r) = 0.0247 px, e(0) = 0.3485 px, e(-r) = 0.6913 px,
a ratio of 0.071 against the condition 0.5."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import path_ref as P  # noqa: E402
import shutter_ref as S  # noqa: E402

FRAME = (360, 640)


def _motion(n, seed):
    rs = np.random.RandomState(seed)
    th = np.deg2rad(0.3 * rs.normal(size=n))
    s = 1.0 + 0.002 * rs.normal(size=n)
    m = np.stack([s * np.cos(th), s * np.sin(th), 3.0 * rs.normal(size=n), 3.0 * rs.normal(size=n)], 1)
    m[0] = (1.0, 0.0, 0.0, 0.0)
    return m


def test_r_zero_is_the_affine_composition():
    field = P.make_field((3, 9, 11, 2), 5, scale=1.03)
    c, s = 1.02 * math.cos(0.03), 1.02 * math.sin(0.03)
    d = np.array([[c, -s, 4.0, s, c, -2.5], list(P.IDENTITY), [1.0, 0.0, -7.0, 0.0, 1.0, 3.0]])
    rts = S.rates(_motion(3, 1))
    want, wtol = P.compose64(field, d, FRAME, return_terms=True)
    got, gtol = S.compose_rows64(field, d, rts, 0.0, FRAME, return_terms=True)
    assert np.array_equal(got, want) and np.array_equal(gtol, wtol)
    # and so are all-zero rates under any r
    got = S.compose_rows64(field, d, np.zeros((3, 2, 4)), 0.8, FRAME)
    assert np.array_equal(got, want)
    # an identity frame is copied only when nothing moves
    assert S.copied(d[1], np.zeros((2, 4)), 0.8) and S.copied(d[1], rts[1], 0.0) and not S.copied(d[1], rts[1], 0.8) and not S.copied(d[0], rts[0], 0.0)
    assert np.abs(S.compose_rows64(field, d, rts, 0.8, FRAME)[1] - field[1]).max() > 1e-4


def test_a_steady_pan_is_sheared_in_closed_form():
    """D = I, a pan of v pixels a frame: x' = x - r v clamp(y / (h0 - 1), -1/2, 1/2), y' = y, on the identity field the composed field itself."""
    h0, w0 = FRAME
    lattice = (7, 9)
    for r in (0.8, -1.0):
        for v in (3.0, -1.25):
            motion = np.tile(np.array([1.0, 0.0, v, 0.0]), (4, 1))
            rts = S.rates(motion)
            assert np.array_equal(rts, np.tile(np.array([0.0, 0.0, v, 0.0]), (4, 2, 1)))
            d = np.tile(np.array(P.IDENTITY), (4, 1))
            p = S.positions64(d, rts, r, lattice, FRAME)
            y, x = np.meshgrid(np.linspace(-0.5 * (h0 - 1), 0.5 * (h0 - 1), lattice[0]), np.linspace(-0.5 * (w0 - 1), 0.5 * (w0 - 1), lattice[1]), indexing="ij")
            want = np.stack([x - r * v * np.clip(y / (h0 - 1), -0.5, 0.5), y], -1)
            assert np.abs(p - want).max() <= 1e-12
            assert abs(abs(p[0, 0, 0, 0] - x[0, 0]) - 0.5 * abs(r * v)) <= 1e-12     # the top row: half the readout away
            got = S.field_positions(S.compose_rows64(S.identity_field(4, lattice), d, rts, r, FRAME), FRAME)
            assert np.abs(got - want).max() <= 1e-4   # (the identity field is float32: 2^-24 of 320 pixels per node)


def test_forward_and_backward_rates_describe_one_velocity():
    """motion[k+1] = (s Rot(f), t) maps frame k+1 into frame k.  The forward row of frame k and the backward row of frame k+1 come from it:
    the same rates of scale and angle, and the translation rate of frame k+1 is that of frame k carried into frame k+1's coordinates by the
    linear part of the inverse map, Rot(-f) / s."""
    m = _motion(9, 2)
    rts = S.rates(m)
    for k in range(8):
        a, b, tx, ty = m[k + 1]
        s, f = math.hypot(a, b), math.atan2(b, a)
        fwd, bwd = rts[k, 0], rts[k + 1, 1]
        assert fwd[0] == bwd[0] == math.log(s) and fwd[1] == bwd[1] == f
        assert (fwd[2], fwd[3]) == (tx, ty)
        carried = np.array([[math.cos(f), math.sin(f)], [-math.sin(f), math.cos(f)]]) @ np.array([tx, ty]) / s
        assert np.abs(bwd[2:] - carried).max() <= 1e-15 * (abs(tx) + abs(ty))
    # a pure translation is the same vector in both frames
    m = np.tile(np.array([1.0, 0.0, 2.0, -1.0]), (3, 1))
    assert np.array_equal(S.rates(m)[:, 0], S.rates(m)[:, 1])


def test_cuts_nan_rows_and_one_frame_scenes():
    m = _motion(10, 3)
    rts = S.rates(m)
    assert np.array_equal(rts[0, 1], rts[0, 0]) and np.array_equal(rts[9, 0], rts[9, 1])      # the ends use their one pair twice
    assert np.array_equal(rts[0, 0], S.forward_rate(m[1])) and np.array_equal(rts[9, 1], S.backward_rate(m[9]))
    assert not S.rates(m[:1]).any() and S.rates(m[:1]).shape == (1, 2, 4) and S.rates(m[:0]).shape == (0, 2, 4)
    other = m.copy()
    other[0] = np.nan                                                                          # row 0 is not read
    assert np.array_equal(S.rates(other), rts)
    a, b = m.copy(), m.copy()
    a[4], b[4] = (np.nan, 0.0, 1.0, np.inf), (1.0, 0.0, 0.0, 0.0)
    assert np.array_equal(S.rates(a), S.rates(b)) and not S.rates(a)[3, 0].any() and not S.rates(a)[4, 1].any()
    cut = S.shutter_rates(m, [4, 5])                                                           # (a scene of one frame between two others)
    assert np.array_equal(cut[:4], S.rates(m[:4])) and not cut[4].any() and np.array_equal(cut[5:], S.rates(m[5:]))
    assert np.array_equal(cut[3, 0], cut[3, 1]) and np.array_equal(cut[5, 1], cut[5, 0])       # no rate reads the pair across a cut
    assert np.array_equal(S.shutter_rates(m), rts)


def test_the_correction_makes_the_frames_rigid_and_the_wrong_sign_does_not():
    e_plus, e_zero, e_minus = S.experiment()
    print("non-rigidity: e(+r) %.4f px, e(0) %.4f px, e(-r) %.4f px, e(+r) / e(0) = %.3f" % (e_plus, e_zero, e_minus, e_plus / e_zero))
    assert e_plus <= 0.5 * e_zero
    assert e_minus > e_zero
    assert e_zero > 0.1   # (there is something to correct)
