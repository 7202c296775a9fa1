"""CPU tests of the float64 restatement of path smoothing (tests/path_ref.py): the definitions' own fixed points, and the experiment that
motivates the feature -- a shaky analytic clip goes in, its measured path is smoothed, and the clip rendered through the corrections
measures steadier by the repository's own metric."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_ref as R  # noqa: E402
import path_ref as P  # noqa: E402


def test_a_constant_translation_is_left_alone_at_every_frame():
    motion = np.tile(np.array([1.0, 0.0, 0.8, -0.3]), (40, 1))
    path, D = P.path_smooth(motion, 4.0)
    assert np.abs(path[:, :2]).max() == 0.0 and np.abs(path[-1, 2:] - 39 * np.array([0.8, -0.3])).max() < 1e-12
    err = np.abs(D - np.array(P.IDENTITY)).max(1)
    print("largest distance from the identity per frame:", err.max(), "at the ends:", err[0], err[-1])
    assert err.max() <= 1e-12


def test_one_and_two_frames():
    path, D = P.path_smooth(np.array([[np.nan] * 4]), 4.0)   # (row 0 is not read)
    assert path.tolist() == [[0.0] * 4] and D.tolist() == [list(P.IDENTITY)]
    m = np.array([[1.0, 0.0, 0.0, 0.0], [1.0, 0.01, 2.0, -1.0]])
    path, D = P.path_smooth(m, 4.0)   # Re = 1: P^[0] = P[0] and P^[1] = P[1] by the odd reflection
    assert np.abs(path[1] - [np.log(np.hypot(1.0, 0.01)), np.arctan2(0.01, 1.0), 2.0, -1.0]).max() < 1e-15
    assert np.abs(D - np.array(P.IDENTITY)).max() <= 1e-12
    assert np.array_equal(P.smooth_path(m, 0.5)[1], path) and P.smooth_path(m, 0.5)[0].shape == (2, 6)


def test_a_nan_row_counts_as_no_motion():
    rs = np.random.RandomState(3)
    m = np.stack([1 + 0.01 * rs.normal(size=12), 0.01 * rs.normal(size=12), rs.normal(size=12), rs.normal(size=12)], 1)
    a, b, c = m.copy(), m.copy(), m.copy()
    a[5] = (np.nan, 0.0, 1.0, 2.0)
    b[5] = (1.0, 0.0, np.inf, 0.0)
    c[5] = (1.0, 0.0, 0.0, 0.0)
    want = P.path_smooth(c, 2.0)
    for got in (P.path_smooth(a, 2.0), P.path_smooth(b, 2.0)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # scenes are smoothed apart: the pair at a cut is not read, and every scene's path starts at zero
    D, path = P.smooth_path(m, 2.0, [7])
    assert np.array_equal(path[7], np.zeros(4)) and np.array_equal(D[7:], P.path_smooth(m[7:], 2.0)[1])


def test_the_scaled_fit_at_one_is_the_plane_fit():
    clip = R.texture_clip(R.planted_path(3, seed=11), 96, 96, seed=3)
    mv, sad, act = R.block_motion(clip, 8)
    want = R.motion_fit(mv, sad, act, 96, 96, 8)
    got = P.motion_fit_scaled(mv, sad, act, 96, 96, 8, scale=(1.0, 1.0))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.isfinite(got[0]).all()


def test_composition_of_an_affine_field_is_exact_and_the_identity_copies():
    fh, fw, frame = 9, 12, (90, 160)
    u, v = np.meshgrid(np.linspace(-1, 1, fw), np.linspace(-1, 1, fh))
    F = np.stack([0.9 * u + 0.1 * v + 0.02, -0.05 * u + 1.1 * v - 0.01], -1)[None]
    kx, ky = (frame[1] - 1) / (fw - 1), (frame[0] - 1) / (fh - 1)
    d = np.array([[1.0, 0.0, -2 * kx, 0.0, 1.0, 3 * ky]])   # a whole-node shift, beyond the lattice on two sides
    out = P.compose64(F, d, frame)
    want = np.stack([0.9 * (u - 2 * 2 / (fw - 1)) + 0.1 * (v + 3 * 2 / (fh - 1)) + 0.02, -0.05 * (u - 2 * 2 / (fw - 1)) + 1.1 * (v + 3 * 2 / (fh - 1)) - 0.01], -1)
    assert np.abs(out[0] - want).max() < 1e-12
    assert np.array_equal(P.compose64(F, np.array([P.IDENTITY]), frame), F)
    assert np.array_equal(P.compose64(F, np.array([[np.nan, 0, 0, 0, 1, 0]]), frame), F)


def test_a_shaky_clip_comes_out_steadier():
    """planted_path(48, seed=5), texture_clip(256 x 256, seed=7), sigma = 4.  Measured by this restatement: stability 0.2129 in and 0.9639
    out; asked for: at most 0.3 in, at least 0.9 out."""
    s_in, s_out = P.experiment(48, 5, 7, 4.0)
    print("stability in %.4f, out %.4f" % (s_in, s_out))
    assert s_in <= 0.3 and s_out >= 0.9
