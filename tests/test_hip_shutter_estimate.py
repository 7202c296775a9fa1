"""GPU tests of the rolling-shutter estimate's kernels (csrc/shutter_estimate.hip; stream.estimate_rolling_shutter) against the float64
restatement tests/shutter_est_ref.py, on the blocks, the motion and the rates that the device itself measured: the terms and the estimate
within the spread of the restatement's own three summation orders, as tests/test_hip_motion.py measures its tolerance; the counts exactly;
the same bits on every run; and the errors.  The shapes are the smallest that take each path: 25 blocks (a partial wave), 289 blocks (more
than one pass over the 256 lanes), a non-square plane in frame pixels, and a clip with two cuts, a NaN row and a pair without enough blocks."""
import functools
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_ref as R  # noqa: E402
import shutter_est_ref as E  # noqa: E402

# name: (T, h, w, radius, pixel_scale, frame_height, cuts)
CASES = {"partial-wave": (8, 96, 96, 8, None, None, None),
         "two-passes": (5, 304, 304, 16, None, None, None),
         "frame-pixels": (8, 96, 128, 8, (10.0, 7.5), 720, None),
         "cuts-nan-few": (16, 96, 96, 8, None, None, [6, 11])}


@functools.lru_cache(maxsize=None)
def _planes(name):
    T, h, w = CASES[name][:3]
    planes = R.texture_clip(R.planted_path(T, seed=11 + T, jitter=True, sigma_px=1.0), h, w, seed=3)
    planes.setflags(write=False)
    return planes


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _measure(name):
    """What the device measured on the case's planes: motion, blocks (and, for the last case, a NaN row and a pair with 7 active blocks)."""
    from pwstablenet_amd.stream import global_motion
    T, h, w, radius, scale, h0, cuts = CASES[name]
    d = torch.from_numpy(np.array(_planes(name))).cuda()
    motion, inl, mv, sad, act = global_motion(d, radius, return_blocks=True, pixel_scale=scale)
    assert torch.isfinite(motion).all() and int(inl[1:].min()) >= 8, name
    if name == "cuts-nan-few":
        motion[14] = math.nan        # takes pairs 13 and 14 of the last scene
        act[8].view(-1)[7:] = 0      # pair 8 keeps 7 blocks that can count
    return motion, mv, sad, act


@pytest.mark.parametrize("name", list(CASES))
def test_terms_and_estimate_agree_with_the_restatement(hip, name):
    """The kernel's order (a lane's blocks in index order, then a butterfly; the rows in index order) against the restatement's forward
    order: at most 16 times the largest spread between the restatement's forward, reverse and pairwise orders on the same inputs, at least
    1e-12.  The counts are equal exactly: no block lies within a relative 1e-3 of its pair's inlier threshold, asserted first."""
    from pwstablenet_amd.stream import estimate_rolling_shutter, shutter_rates
    T, h, w, radius, scale, h0, cuts = CASES[name]
    motion, mv, sad, act = _measure(name)
    est, terms = estimate_rolling_shutter(motion, mv, sad, act, (h, w), radius=radius, pixel_scale=scale, scene_cuts=cuts, frame_height=h0,
                                          return_terms=True)
    assert est.is_cuda and est.dtype == torch.float64 and est.shape == (4,) and terms.dtype == torch.float64 and terms.shape == (T, 4)
    rates = shutter_rates(motion, scene_cuts=cuts)
    blocks = [x.cpu().numpy() for x in (mv, sad, act)]
    kw = dict(radius=radius, scale=scale or (1.0, 1.0), h0=h0, scene_cuts=cuts)
    margins = []
    want = E.terms(*blocks, motion.cpu().numpy(), rates.cpu().numpy(), h, w, margins=margins, **kw)
    assert margins and min(margins) > 1e-3, (name, min(margins))
    want_est = E.estimate(want)
    spread, spread_est = 0.0, 0.0
    for order in ("reverse", "pairwise"):
        other = E.terms(*blocks, motion.cpu().numpy(), rates.cpu().numpy(), h, w, order=order, **kw)
        assert np.array_equal(other[:, 3], want[:, 3]), name
        spread = max(spread, float(np.abs(other - want).max()))
        spread_est = max(spread_est, float(np.abs(E.estimate(other, order)[:3] - want_est[:3]).max()))
    tol, tol_est = max(16.0 * spread, 1e-12), max(16.0 * spread_est, 1e-12)
    got, got_est = terms.cpu().numpy(), est.cpu().numpy()
    err, err_est = float(np.abs(got - want).max()), float(np.abs(got_est[:3] - want_est[:3]).max())
    print(name, "terms: spread", spread, "kernel against forward", err, "tolerance", tol, "| estimate: spread", spread_est, "kernel", err_est,
          "tolerance", tol_est, "| smallest margin", min(margins), "counts", want[:, 3].tolist(), "estimate", got_est.tolist())
    assert np.array_equal(got[:, 3], want[:, 3]), name
    assert err <= tol and err_est <= tol_est and got_est[3] == want_est[3], (name, err, tol, err_est, tol_est)
    usable = E.usable_pairs(motion.cpu().numpy(), cuts)
    assert not got[~usable].any() and (got[usable, 3] >= 8).sum() >= 2, name   # zero rows where the definition says so, real ones elsewhere
    if name == "cuts-nan-few":   # scenes [0, 6), [6, 11), [11, 16): pairs 2 .. 4, 8 .. 9, 13 .. 14; the NaN row takes 13 and 14, pair 8 has 7 blocks
        assert [k for k in range(T) if got[k].any()] == [2, 3, 4, 9]
    assert math.isfinite(got_est[0]) and got_est[1] > 0.0 and got_est[2] > 0.0
    # the same bits on every run
    again = estimate_rolling_shutter(motion, mv, sad, act, (h, w), radius=radius, pixel_scale=scale, scene_cuts=cuts, frame_height=h0,
                                     return_terms=True)
    assert torch.equal(_bits(again[0]), _bits(est)) and torch.equal(_bits(again[1]), _bits(terms)), name
    alone = estimate_rolling_shutter(motion, mv, sad, act, (h, w), radius=radius, pixel_scale=scale, scene_cuts=cuts, frame_height=h0)
    assert torch.equal(_bits(alone), _bits(est))


def test_short_clips_have_no_usable_pair(hip):
    from pwstablenet_amd.stream import estimate_rolling_shutter
    motion, mv, sad, act = _measure("partial-wave")
    for T in (0, 1, 3):
        est, terms = estimate_rolling_shutter(motion[:T], mv[:T], sad[:T], act[:T], (96, 96), radius=8, return_terms=True)
        assert terms.shape == (T, 4) and not terms.any()
        assert math.isnan(float(est[0])) and float(est[1]) == math.inf and est[2:].tolist() == [0.0, 0.0]
    est, terms = estimate_rolling_shutter(motion[:4], mv[:4], sad[:4], act[:4], (96, 96), radius=8, return_terms=True)
    assert [k for k in range(4) if terms[k].any()] == [2]   # T = 4: pair 2 has a real pair on both sides


def test_frame_height_defaults_to_the_planes_height_in_motions_pixels(hip):
    from pwstablenet_amd.stream import estimate_rolling_shutter
    T, h, w, radius, scale, h0, _ = CASES["frame-pixels"]
    motion, mv, sad, act = _measure("frame-pixels")
    a = estimate_rolling_shutter(motion, mv, sad, act, (h, w), radius=radius, pixel_scale=scale)
    b = estimate_rolling_shutter(motion, mv, sad, act, (h, w), radius=radius, pixel_scale=scale, frame_height=h * scale[1])
    assert h * scale[1] == h0 and torch.equal(_bits(a), _bits(b))


def test_errors(hip):
    from pwstablenet_amd.stream import estimate_rolling_shutter as est
    motion, mv, sad, act = _measure("partial-wave")
    ok = dict(radius=8)
    est(motion, mv, sad, act, (96, 96), **ok)
    for bad in (motion.float(), motion[:, :3], motion.cpu(), motion.cpu().numpy(), motion[0]):
        with pytest.raises(ValueError, match="motion"):
            est(bad, mv, sad, act, (96, 96), **ok)
    with pytest.raises(ValueError, match="mv"):
        est(motion, mv.int(), sad, act, (96, 96), **ok)
    with pytest.raises(ValueError, match="mv"):
        est(motion, mv[:-1], sad, act, (96, 96), **ok)
    with pytest.raises(ValueError, match="sad"):
        est(motion, mv, sad[..., :4], act, (96, 96), **ok)
    with pytest.raises(ValueError, match="sad"):
        est(motion, mv, sad.cpu(), act, (96, 96), **ok)
    with pytest.raises(ValueError, match="activity"):
        est(motion, mv, sad, torch.zeros((8, 5, 10), dtype=torch.int32, device="cuda")[:, :, ::2], (96, 96), **ok)   # not contiguous
    with pytest.raises(ValueError, match="mv"):   # blocks of another lattice
        est(motion, mv, sad, act, (112, 96), **ok)
    with pytest.raises(ValueError, match="plane_hw"):
        est(motion, mv, sad, act, 96, **ok)
    for radius in (0, 17):
        with pytest.raises(ValueError, match="radius"):
            est(motion, mv, sad, act, (96, 96), radius=radius)
    with pytest.raises(ValueError, match="no 16 x 16 block"):
        est(motion, mv, sad, act, (31, 96), **ok)
    for scale in ((0.0, 1.0), (1.0, float("nan")), (1.0,), "ab"):
        with pytest.raises(ValueError, match="pixel_scale"):
            est(motion, mv, sad, act, (96, 96), pixel_scale=scale, **ok)
    for fh in (1.0, 0, -5, float("nan"), float("inf"), "tall"):
        with pytest.raises(ValueError, match="frame_height"):
            est(motion, mv, sad, act, (96, 96), frame_height=fh, **ok)
    for cuts in ([0], [8], [5, 5], [6, 4], ["a"]):
        with pytest.raises(ValueError, match="scene_cuts"):
            est(motion, mv, sad, act, (96, 96), scene_cuts=cuts, **ok)
    L, P = hip.lib(), hip.ptr
    rates = torch.zeros((8, 2, 4), dtype=torch.float64, device="cuda")
    terms, out4 = torch.zeros((8, 4), dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
    args = lambda **k: [k.get("mv", P(mv)), P(sad), P(act), k.get("motion", P(motion)), P(rates), k.get("n", 8), k.get("h", 96), 96,  # noqa: E731
                        k.get("radius", 8), 2000, k.get("sx", 1.0), 1.0, k.get("h0", 96.0), k.get("terms", P(terms)), None]
    for kw, word in ((dict(radius=0), b"radius"), (dict(radius=17), b"radius"), (dict(h=20), b"no 16 x 16 block"), (dict(n=-1), b"bad shape"),
                     (dict(sx=0.0), b"pixel scale"), (dict(sx=float("nan")), b"pixel scale"), (dict(h0=1.0), b"frame height"),
                     (dict(h0=float("nan")), b"frame height"), (dict(mv=None), b"NULL"), (dict(terms=None), b"NULL"),
                     (dict(motion=hip.ctypes.c_void_p(motion.data_ptr() + 4)), b"aligned"),
                     (dict(mv=hip.ctypes.c_void_p(mv.data_ptr() + 2)), b"aligned")):
        assert L.pws_shutter_terms(*args(**kw)) == -22 and word in L.pws_last_error(), kw
    assert L.pws_shutter_terms(None, None, None, None, None, 0, 96, 96, 8, 2000, 1.0, 1.0, 96.0, None, None) == 0
    assert L.pws_shutter_terms(*args()) == 0
    assert L.pws_shutter_estimate(P(terms), -1, P(out4), None) == -22 and b"bad shape" in L.pws_last_error()
    assert L.pws_shutter_estimate(P(terms), 8, None, None) == -22 and b"NULL" in L.pws_last_error()
    assert L.pws_shutter_estimate(None, 8, P(out4), None) == -22 and b"NULL" in L.pws_last_error()
    assert L.pws_shutter_estimate(hip.ctypes.c_void_p(terms.data_ptr() + 4), 7, P(out4), None) == -22 and b"aligned" in L.pws_last_error()
    assert L.pws_shutter_estimate(P(terms), 8, P(out4), None) == 0
    torch.cuda.synchronize()
