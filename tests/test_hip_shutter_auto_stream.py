"""GPU tests of VideoStabilizer(smooth=sigma, rolling_shutter="auto"): the frames are, bit for bit, those of a second stabiliser constructed
with the number that the first one chose (``rolling_shutter_used``), for bgr24 and nv12, with and without cuts, with the gate open and at its
default; ``shutter_estimate`` is ``estimate_rolling_shutter`` called by hand on the same measured motion; a still clip makes the gate choose
0.0 and gives the frames of smoothing alone; and the arguments that cannot work are refused.  tests/test_hip_shutter_stream.py's identity
generator (ngf = 16, the head's bias at the identity, align_corners=True) and its shaky textured scene, 32 frames of 640 x 320, batch 8,
chunk 16."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pwstablenet_amd import synth  # noqa: E402

T, H, W = 32, 320, 640
SIGMA = 4.0
CHUNK = 16


@pytest.fixture(scope="module")
def net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    sd = {"module." + k: torch.from_numpy(v.copy()) for k, v in synth.make_weights("W1", seed=123, ngf=16)}
    sd["module.linear.mpconv.0.weight"].zero_()   # the head's bias at identity and nothing else feeding the field
    sd["module.linear.mpconv.0.bias"].copy_(torch.from_numpy(synth.IDENTITY_THETA))
    sd["module.out.mpconv.0.weight"].zero_()
    sd["module.out.mpconv.0.bias"].zero_()
    g = define_G(31, 2, 16, "normal", 0.02)
    g.load_state_dict(sd)
    g.module.align_corners = True
    return g.cuda()


def _texture_u8(n, h, w, seed, lam=(14.0, 90.0), sigma=3.0):
    """tests/test_hip_smooth_stream.py's shaky textured scene, (n, h, w) uint8: twelve sinusoids under a pan of (1.0, 0.4) pixel a frame plus
    Gaussian jitter of the pose (translations only)."""
    rs = np.random.RandomState(seed)
    k = 12
    wl, ang, ph = rs.uniform(lam[0], lam[1], k), rs.uniform(0, 2 * np.pi, k), rs.uniform(0, 2 * np.pi, k)
    kx, ky = 2 * np.pi / wl * np.cos(ang), 2 * np.pi / wl * np.sin(ang)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    a = kx[:, None, None] * xx + ky[:, None, None] * yy + ph[:, None, None]
    sa, ca = np.sin(a).astype(np.float32).reshape(k, -1), np.cos(a).astype(np.float32).reshape(k, -1)
    t = np.arange(n)
    tx, ty = 1.0 * t + rs.normal(0, sigma, n), 0.4 * t + rs.normal(0, sigma, n)
    phi = kx[None] * tx[:, None] + ky[None] * ty[:, None]
    v = np.cos(phi).astype(np.float32) @ sa + np.sin(phi).astype(np.float32) @ ca
    return np.clip(np.rint(127.5 + 127.5 * 0.13 * v), 0, 255).astype(np.uint8).reshape(n, h, w)


@pytest.fixture(scope="module")
def clips():
    base = _texture_u8(T, H, W, 21)
    rs = np.random.RandomState(21)
    col = np.stack([base * 0.9, base * 1.0, base * 0.8], -1) + rs.randint(-3, 4, (T, H, W, 3))
    uv = synth.smooth_frames_u8(1, T, H // 2, W, 23)[0] // 2 + 64
    return {"bgr24": torch.from_numpy(np.clip(col, 0, 255).astype(np.uint8)).cuda(),
            "nv12": torch.from_numpy(np.concatenate([_texture_u8(T, H, W, 22), uv], 1)).cuda()}


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)))


# (format, run_video's arguments, shutter_max_se): 1e9 opens the gate, so that a number other than 0 is what the second stabiliser gets
CASES = [("bgr24", {}, 1e9), ("nv12", {}, 1e9), ("bgr24", {"scene_cuts": [13]}, 1e9), ("nv12", {"scene_cuts": [13]}, None)]
IDS = ["%s-%s-%s" % (f, "-".join(sorted(k)) or "plain", "open" if m else "default") for f, k, m in CASES]


@pytest.mark.parametrize("fmt,call,max_se", CASES, ids=IDS)
def test_auto_is_the_stabiliser_with_the_number_it_chose(hip, net, clips, fmt, call, max_se):
    from pwstablenet_amd.stream import VideoStabilizer
    src = clips[fmt]
    kw = {} if max_se is None else {"shutter_max_se": max_se}
    vs = VideoStabilizer(net, batch=8, smooth=SIGMA, rolling_shutter="auto", **kw)
    assert vs.rolling_shutter == "auto" and vs.shutter_max_se == (0.02 if max_se is None else max_se)
    assert vs.shutter_estimate is None and vs.rolling_shutter_used is None
    got = vs.run_video(src, chunk=CHUNK, pixel_format=fmt, **call)
    est, used = vs.shutter_estimate, vs.rolling_shutter_used
    assert est.is_cuda and est.dtype == torch.float64 and est.shape == (4,) and isinstance(used, float)
    r_hat, se, energy, blocks = est.tolist()
    print(fmt, call, "estimate", est.tolist(), "used", used)
    assert math.isfinite(r_hat) and se > 0.0 and energy > 0.0 and blocks >= 8   # a shaky clip: the regressor has energy
    assert used == (min(1.0, max(-1.0, r_hat)) if se <= vs.shutter_max_se else 0.0)
    if max_se is not None:
        assert used != 0.0
    ref = VideoStabilizer(net, batch=8, smooth=SIGMA, rolling_shutter=used)
    want = ref.run_video(src, chunk=CHUNK, pixel_format=fmt, **call)
    assert ref.shutter_estimate is None and ref.rolling_shutter_used is None
    assert got.shape == want.shape and torch.equal(got, want)
    for name in ("smooth_motion", "smooth_inliers", "smooth_path", "smooth_correction", "smooth_uncovered", "shutter_rates"):
        assert _same(getattr(vs, name), getattr(ref, name)), name
    # a call with a number leaves nothing of "auto" behind
    vs.rolling_shutter = 0.0
    vs.run_video(src, chunk=CHUNK, pixel_format=fmt, **call)
    assert vs.shutter_estimate is None and vs.rolling_shutter_used is None


@pytest.mark.parametrize("cuts", [None, [13]], ids=["plain", "cuts"])
def test_the_estimate_is_the_by_hand_call(hip, net, clips, cuts):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    src = clips["bgr24"]
    vs = S.VideoStabilizer(net, batch=8, smooth=SIGMA, rolling_shutter="auto")
    vs.run_video(src, chunk=CHUNK, scene_cuts=cuts)
    planes = S.window_planes(src)
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    half = vs.period // 2
    with torch.no_grad():
        for cs in range(0, T, CHUNK):   # pass 1's generator calls: per chunk, on the chunk's planes and what its windows reach
            ce = min(T, cs + CHUNK)
            hl, hr = min(half, cs), min(half, T - ce)
            sc = [t - (cs - hl) for t in (cuts or []) if cs - hl < t < ce + hr] or None
            vs._fields(planes[cs - hl:ce + hr], hl, hr, fields[cs:ce], sc)
    seen = PF.grid_sample(planes.unsqueeze(1), fields, align_corners=vs.align_corners).squeeze(1)
    scale = (W / 256.0, H / 256.0)
    motion, inl, mv, sad, act = S.global_motion(seen, pixel_scale=scale, return_blocks=True)
    assert _same(motion, vs.smooth_motion) and _same(inl, vs.smooth_inliers)
    want = S.estimate_rolling_shutter(motion, mv, sad, act, (256, 256), pixel_scale=scale, scene_cuts=cuts, frame_height=H)
    assert _same(vs.shutter_estimate, want)


def test_a_still_clip_is_left_to_smoothing_alone(hip, net, clips):
    from pwstablenet_amd.stream import VideoStabilizer
    still = clips["bgr24"][:1].expand(T, H, W, 3).contiguous()
    vs = VideoStabilizer(net, batch=8, smooth=SIGMA, rolling_shutter="auto", shutter_max_se=1e9)
    got = vs.run_video(still, chunk=CHUNK)
    r_hat, se, energy, _ = vs.shutter_estimate.tolist()
    assert math.isnan(r_hat) and se == math.inf and energy == 0.0   # no motion, no acceleration: nothing to regress on
    assert vs.rolling_shutter_used == 0.0 and vs.shutter_rates is None
    plain = VideoStabilizer(net, batch=8, smooth=SIGMA)
    assert torch.equal(got, plain.run_video(still, chunk=CHUNK)) and _same(vs.smooth_correction, plain.smooth_correction)


class _Stub:
    """A generator stand-in for the argument checks, which come before any generator call."""

    def __call__(self, x, is_training):
        raise AssertionError("the generator must not run")


def test_arguments_that_cannot_work_are_refused(hip):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    for bad in ("Auto", "estimate", ""):
        with pytest.raises(ValueError, match="rolling_shutter"):
            S.VideoStabilizer(_Stub(), batch=8, smooth=SIGMA, rolling_shutter=bad)
    with pytest.raises(ValueError, match="smooth"):
        S.VideoStabilizer(_Stub(), batch=8, rolling_shutter="auto")
    with pytest.raises(ValueError, match="smooth"):
        S.VideoStabilizer(_Stub(), batch=8, smooth=0.0, rolling_shutter="auto")
    for bad in (-0.01, float("nan"), "wide", None):
        with pytest.raises(ValueError, match="shutter_max_se"):
            S.VideoStabilizer(_Stub(), batch=8, smooth=SIGMA, rolling_shutter="auto", shutter_max_se=bad)
    frames = torch.zeros((34, H, W, 3), dtype=torch.uint8, device="cuda")
    vs = S.VideoStabilizer(_Stub(), batch=8, smooth=SIGMA, rolling_shutter="auto")
    with pytest.raises(ValueError, match="whole clip"):
        vs.run_video(frames, halo_left=2)
    for borders in ("keep", "mosaic"):
        with pytest.raises(ValueError, match=borders):
            S.VideoStabilizer(_Stub(), batch=8, smooth=SIGMA, rolling_shutter="auto", borders=borders).run_video(frames)
    vs.rolling_shutter = "estimate"   # (set after construction: the call refuses)
    with pytest.raises(ValueError, match="rolling_shutter"):
        vs.run_video(frames)
    vs.rolling_shutter, vs.shutter_max_se = "auto", float("nan")
    with pytest.raises(ValueError, match="shutter_max_se"):
        vs.run_video(frames)
    vs.shutter_max_se, vs.smooth = 0.02, 0.0
    with pytest.raises(ValueError, match="smooth"):
        vs.run_video(frames)
    # compose_fields and limit_path keep taking numbers only
    field = torch.zeros((2, 8, 8, 2), device="cuda")
    d = torch.tensor([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * 2, dtype=torch.float64, device="cuda")
    rates = torch.zeros((2, 2, 4), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="rolling_shutter"):
        PF.compose_fields(field, d, (64, 64), rates=rates, rolling_shutter="auto")
    with pytest.raises(ValueError, match="rolling_shutter"):
        S.limit_path(d, field, (64, 64), 0.9, rates=rates, rolling_shutter="auto")
