"""CPU tests of tests/keep_ref.py, the float64 restatement the GPU tests of the "keep" borders are held to: coverage of fields whose
coordinates are exact, a recurrence worked out by hand, the initial frame's read rules, and the condition on the GPU tests' fields (at most
1 % of a case's pixels within delta of a coverage threshold, delta = 4 x the largest fp32 coordinate error of that case)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bicubic_ref as B  # noqa: E402
import keep_ref as K  # noqa: E402


def exact_identity(n, h, w, ac):
    """A field at the plane's own size whose coordinates are the pixel's own, exactly: align_corners False at power-of-two sizes (the base
    grid (2 i + 1) / size - 1), True at sizes 2^k + 1 (i / 2^(k-1) - 1)."""
    if not ac:
        return B.affine_field(n, h, w)
    xs, ys = np.arange(w, dtype=np.float32) * np.float32(2.0 / (w - 1)) - 1, np.arange(h, dtype=np.float32) * np.float32(2.0 / (h - 1)) - 1
    gx, gy = np.meshgrid(xs, ys, indexing="xy")
    return np.broadcast_to(np.stack([gx, gy], -1), (n, h, w, 2)).astype(np.float32)


@pytest.mark.parametrize("ac,hw", [(False, (16, 32)), (True, (17, 9))])
def test_identity_covers_everything_and_bicubic_leaves_a_rim(ac, hw):
    h, w = hw
    field = exact_identity(2, h, w, ac)
    ix, iy = K.coordinates(field, h, w, ac)
    assert np.array_equal(ix[0], np.broadcast_to(np.arange(w, dtype=np.float64), (h, w)))
    assert np.array_equal(iy[0], np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w)))
    cov0, dist0 = K.coverage(field, h, w, ac, 0)
    assert cov0.all() and dist0.min() == 0.0
    cov1, _ = K.coverage(field, h, w, ac, 1)
    rim = np.ones((h, w), bool)
    rim[1:-1, 1:-1] = False
    assert np.array_equal(cov1[0], ~rim) and np.array_equal(cov1[1], ~rim)


@pytest.mark.parametrize("k", [2.0, 2.5, -3.0, -0.5])
def test_shift_uncovers_the_expected_columns(k):
    """ix = ox + k exactly (a 32-wide plane, align_corners False, shift 2 k / 32)."""
    h, w = 8, 32
    field = B.affine_field(1, h, w, shift=(2 * k / w, 0.0))
    ix, _ = K.coordinates(field, h, w, False)
    assert np.array_equal(ix[0, 0], np.arange(w) + k)
    for m in (0, 1):
        cov, dist = K.coverage(field, h, w, False, m)
        want = (np.arange(w) + k >= m) & (np.arange(w) + k <= w - 1 - m)
        rows = np.arange(h)
        want2 = want[None, :] & ((rows >= m) & (rows <= h - 1 - m))[:, None]
        assert np.array_equal(cov[0], want2)
        assert (~cov[0]).sum() > 0
        assert dist[0, 3].min() == (0.0 if k == int(k) else 0.5)   # (an inner row: iy is 2 away from its thresholds)


def test_nan_is_not_covered():
    field = B.affine_field(1, 8, 8)
    field[0, 3, 4, 0] = np.nan
    cov, _ = K.coverage(field, 8, 8, False, 0)
    assert not cov[0, 3, 4] and cov[0, 0, 0] and cov[0, 7, 7]


def test_three_frame_recurrence_by_hand():
    """A 2 x 4 one-channel plane (as the Y plane of a 4:2:0 frame would be), align_corners False, fields at the plane's own size: frame 0
    shifted by +1 pixel (column 3 uncovered), frame 1 by -1 (column 0), then a cut, frame 2 by +2 (columns 2, 3)."""
    h, w = 2, 4
    field = np.concatenate([B.affine_field(1, h, w, shift=(2 * k / w, 0.0)) for k in (1.0, -1.0, 2.0)])
    cov, _ = K.coverage(field, h, w, False, 0)
    assert np.array_equal(cov[:, 0], np.array([[1, 1, 1, 0], [0, 1, 1, 1], [1, 1, 0, 0]], bool)) and np.array_equal(cov[:, 0], cov[:, 1])
    warped = np.stack([np.full((h, w), v, np.uint8) for v in (10, 20, 30)])
    src = np.arange(3 * h * w, dtype=np.uint8).reshape(3, h, w) + 100
    out = np.empty_like(warped)
    for t in range(3):
        prev = K.initial_frame(src[t], "nv12", True) if t in (0, 2) else out[t - 1]
        out[t] = K.step(prev, warped[t], cov[t])
    assert np.array_equal(out[0], [[10, 10, 10, 103], [10, 10, 10, 107]])
    assert np.array_equal(out[1], [[10, 20, 20, 20], [10, 20, 20, 20]])          # column 0: frame 0's OUTPUT, not frame 1's source
    assert np.array_equal(out[2], [[30, 30, 118, 119], [30, 30, 122, 123]])      # after the cut: frame 2's source, nothing of frame 1


def test_keep_clip_matches_the_steps():
    h, w = 8, 16
    rs = np.random.RandomState(0)
    field = K.field_case("shift", 8, 0)
    for fmt, shape, dt in (("bgr24", (K.T, h, w, 3), np.uint8), ("nv12", (K.T, h * 3 // 2, w), np.uint8), ("i010", (K.T, h * 3 // 2, w), np.uint16)):
        warped, src = rs.randint(0, 256, shape).astype(dt), rs.randint(0, 256, shape).astype(dt)
        out = K.keep_clip(warped, field, src, fmt, False, 0, scene_cuts=(2,))
        cov, _ = K.packed_coverage(field, fmt, h, w, False, 0)
        assert not cov.all() and cov.any()
        for t in range(K.T):
            prev = src[t] if t in (0, 2) else out[t - 1]
            assert np.array_equal(out[t], np.where(cov[t], warped[t], prev))
        assert ((out == warped) | (out == src) | (out == np.roll(out, 1, 0))).all()


def test_initial_frame_read_rules():
    rs = np.random.RandomState(1)
    words = rs.randint(0, 65536, (6, 8)).astype(np.uint16)
    p = K.initial_frame(words, "p010", True)
    assert np.array_equal(p, (words >> 6) << 6) and (p & 63 == 0).all() and (words & 63 != 0).any()
    i = K.initial_frame(words, "i010", True)
    assert i.max() == 1023 and np.array_equal(i, np.where(words > 1023, 1023, words)) and (words > 1023).any()
    small = np.array([[0, 1, 1023, 1024, 65535]], np.uint16)
    assert K.initial_frame(small, "i010", True).tolist() == [[0, 1, 1023, 1023, 1023]]
    assert K.initial_frame(small, "p010", True).tolist() == [[0, 0, 960, 1024, 65472]]
    for fmt in ("p010", "i010", "nv12", "bgr24"):   # an earlier OUTPUT frame is taken as it is
        assert np.array_equal(K.initial_frame(words, fmt, False), words)
    bgr = rs.randint(0, 256, (4, 4, 3)).astype(np.uint8)
    assert np.array_equal(K.initial_frame(bgr, "bgr24", True, swap_rb=True), bgr[..., ::-1])
    assert np.array_equal(K.initial_frame(bgr, "bgr24", True), bgr)
    assert np.array_equal(K.initial_frame(bgr, "nv12", True), bgr)


def test_fp32_coordinates_follow_float64():
    """The numpy float32 evaluation of the kernels' sequence reproduces exact coordinates exactly and stays within a few ulps of the
    plane's width elsewhere."""
    field = B.affine_field(2, 16, 32)
    x32, y32 = K.coordinates32(field, 16, 32, False)
    x64, y64 = K.coordinates(field, 16, 32, False)
    assert np.array_equal(x32.astype(np.float64), x64) and np.array_equal(y32.astype(np.float64), y64)
    assert K.fp32_error(K.field_case("smooth", 8, 3), 18, 24, True) < 24 * 2.0 ** -20


def gpu_cases():
    for h, w, fs in K.SHAPES:
        for case in K.FIELDS:
            yield h, w, fs, case
    yield K.BIG + ("smooth",)
    yield K.BIG + ("shift",)


@pytest.mark.parametrize("h,w,fs,case", list(gpu_cases()))
def test_condition_on_the_gpu_fields(h, w, fs, case):
    """Every field tests/test_hip_keep.py uses leaves at most 1 % of each plane's pixels within delta of a threshold, by the restatement
    alone; and each case is what its name says."""
    field = K.field_case(case, fs, seed=w)
    for ac in (False, True):
        for ph, pw in ((h, w), (h // 2, w // 2)):
            delta = K.FACTOR * K.fp32_error(field, ph, pw, ac)
            if case != "outside":
                assert delta < 1e-2, delta   # (|coordinate| ~ 1e4 w there: the error is large and so is every distance)
            for m in (0, 1):
                cov, dist = K.coverage(field, ph, pw, ac, m)
                share = float((dist <= delta).mean())
                print("%dx%d %s ac=%d m=%d: fp32 error %.3g, delta %.3g, undecided %.4f, uncovered %.3f" % (ph, pw, case, ac, m, delta / K.FACTOR, delta, share,
                                                                                                         1 - cov.mean()))
                assert share <= K.CAP, share
                if case == "identity":
                    assert cov.all() or m == 1
                elif case == "outside":
                    assert not cov.any()
                elif case == "smooth":
                    assert not cov.all() and cov.any()
                    if (ph, pw, fs) == K.BIG:
                        assert 1 - cov.mean() > 0.01   # a rim on every side
                        assert not cov[:, 0].all() and not cov[:, -1].all() and not cov[:, :, 0].all() and not cov[:, :, -1].all()
                else:   # a wedge on two sides, the opposite two in odd frames
                    assert 0.02 < 1 - cov.mean() < 0.9
                    assert not cov[0, :, -1].any() and not cov[0, 0, :].any() and cov[0, -2, 1] and not cov[1, :, 0].any() and not cov[1, -1, :].any()
