"""GPU tests of the motion fit in frame pixels (csrc/motion.hip pws_motion_fit_scaled; stream.global_motion(pixel_scale=)) against the float64
restatement tests/path_ref.py: scale (1, 1) is pws_motion_fit bit for bit, scale (5, 2.8125) -- a 1280 x 720 frame's 256 x 256 planes -- agrees
within the spread of the restatement's own three summation orders, as tests/test_hip_motion.py measures its tolerance.  6 frames of 96 x 96,
radius 8: 5 x 5 blocks."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_ref as R  # noqa: E402
import path_ref as P  # noqa: E402

N, H, W, RADIUS = 6, 96, 96, 8
SCALE = (5.0, 2.8125)


@functools.lru_cache(maxsize=None)
def _clip():
    planes = R.texture_clip(R.planted_path(N, seed=11, jitter=True), H, W, seed=3)
    planes.setflags(write=False)
    return planes


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def test_scale_one_is_the_plane_fit_bit_for_bit(hip):
    from pwstablenet_amd.stream import global_motion
    d = torch.from_numpy(np.array(_clip())).cuda()
    want, want_inl = global_motion(d, RADIUS)
    got, got_inl = global_motion(d, RADIUS, pixel_scale=(1, 1))
    assert torch.isfinite(want).all() and int(want_inl[1:].min()) >= 8
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(got_inl, want_inl)
    # and the plane fit is still the restatement's, as tests/test_hip_motion.py holds it
    blocks = R.block_motion(_clip(), RADIUS)
    ref, ref_inl = R.motion_fit(*blocks, H, W, RADIUS)
    assert np.abs(want.cpu().numpy() - ref).max() <= 1e-12 and np.array_equal(want_inl.cpu().numpy(), ref_inl)


def test_scaled_fit_agrees_with_the_restatement_within_its_own_summation_spread(hip):
    """The kernel's order (a lane's blocks in index order, then a butterfly) against the restatement's forward order: at most 16 times the
    largest spread between the restatement's forward, reverse and pairwise orders, at least 1e-12 relative to the scale's magnitude (the
    sums are in frame pixels: 5 times the plane's).  The inlier counts are equal exactly: no block lies within a relative 1e-3 of a round's
    threshold, asserted first."""
    from pwstablenet_amd.stream import global_motion
    planes = _clip()
    d = torch.from_numpy(np.array(planes)).cuda()
    motion, inl, mv, sad, act = global_motion(d, RADIUS, return_blocks=True, pixel_scale=SCALE)
    blocks = [x.cpu().numpy() for x in (mv, sad, act)]
    assert all(np.array_equal(a, b) for a, b in zip(blocks, R.block_motion(planes, RADIUS)))
    margins = []
    want, want_inl = P.motion_fit_scaled(*blocks, H, W, RADIUS, scale=SCALE, order="forward", margins=margins)
    assert np.isfinite(want).all() and margins and min(margins) > 1e-3, min(margins)
    others = [P.motion_fit_scaled(*blocks, H, W, RADIUS, scale=SCALE, order=order) for order in ("reverse", "pairwise")]
    assert all(np.array_equal(i, want_inl) for _, i in others)
    spread = max(float(np.abs(m - want).max()) for m, _ in others)
    tol = max(16.0 * spread, 1e-12 * max(SCALE))
    got = motion.cpu().numpy()
    err = float(np.abs(got - want).max())
    print("spread of the restatement's orders", spread, "kernel against forward", err, "tolerance", tol, "smallest margin", min(margins),
          "inliers", want_inl.tolist())
    assert err <= tol
    assert np.array_equal(inl.cpu().numpy(), want_inl) and got[0].tolist() == [1.0, 0.0, 0.0, 0.0] and int(inl[0]) == 0
    again = global_motion(d, RADIUS, pixel_scale=SCALE)
    assert torch.equal(_bits(again[0]), _bits(motion)) and torch.equal(again[1], inl)
    # the fit is in frame pixels: over a lattice that is symmetric about the centre the translation is the blocks' mean vector, so it is
    # the plane fit's times the axis's scale up to the few blocks the two fits drop differently (a tenth of a plane pixel is allowed;
    # the restatement measures 0.03 and 0.04 of one)
    plane = global_motion(d, RADIUS)[0].cpu().numpy()
    assert np.abs(got[1:, 2] - SCALE[0] * plane[1:, 2]).max() <= 0.1 * SCALE[0] and np.abs(got[1:, 3] - SCALE[1] * plane[1:, 3]).max() <= 0.1 * SCALE[1]


def test_scale_errors(hip):
    from pwstablenet_amd.stream import global_motion
    x = torch.from_numpy(np.array(_clip())).cuda()
    for bad in ((0.0, 1.0), (1.0, -2.0), (float("nan"), 1.0), (float("inf"), 1.0), (1.0,), "ab", 3.0):
        with pytest.raises(ValueError, match="pixel_scale"):
            global_motion(x, RADIUS, pixel_scale=bad)
    L, Pt = hip.lib(), hip.ptr
    mv, sad, act = (torch.zeros(s, dtype=t, device="cuda") for s, t in (((3, 3, 3, 2), torch.int16), ((3, 3, 3, 5), torch.int32), ((3, 3, 3), torch.int32)))
    motion, inl = torch.zeros((3, 4), dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    for sx, sy in ((0.0, 1.0), (1.0, float("nan")), (-1.0, 1.0), (1.0, float("inf"))):
        assert L.pws_motion_fit_scaled(Pt(mv), Pt(sad), Pt(act), 3, 64, 64, 8, 2000, sx, sy, Pt(motion), Pt(inl), None) == -22
        assert b"pixel scale" in L.pws_last_error()
    assert L.pws_motion_fit_scaled(Pt(mv), Pt(sad), Pt(act), 3, 64, 64, 0, 2000, 1.0, 1.0, Pt(motion), Pt(inl), None) == -22 and b"radius" in L.pws_last_error()
    assert L.pws_motion_fit_scaled(None, None, None, 0, 64, 64, 8, 2000, 2.0, 3.0, None, None, None) == 0
