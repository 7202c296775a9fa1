"""GPU tests of rolling-shutter correction in the streaming stabiliser, VideoStabilizer(smooth=sigma, rolling_shutter=r): r = 0 is the
stabiliser without the argument bit for bit; with r = 0.8 the frames are those assembled by hand from the same steps -- kept fields ->
grid_sample of the planes -> global_motion in frame pixels -> smooth_path -> shutter_rates -> compose_fields(rates=, rolling_shutter=) ->
the format's fused warp -- bit for bit, also under scene cuts and zoom="auto"; and the arguments that cannot work are refused.
tests/test_hip_smooth_stream.py's identity generator (ngf = 16, the head's bias at the identity, align_corners=True) and its shaky
textured scene, 32 frames of 640 x 320, batch 8, chunk 16."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pwstablenet_amd import synth  # noqa: E402

T, H, W = 32, 320, 640
SIGMA, R = 4.0, 0.8
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


@pytest.mark.parametrize("fmt", ["bgr24", "nv12"])
def test_zero_is_the_stabiliser_without_the_argument(hip, net, clips, fmt):
    from pwstablenet_amd.stream import VideoStabilizer
    plain = VideoStabilizer(net, batch=8, smooth=SIGMA)
    zero = VideoStabilizer(net, batch=8, smooth=SIGMA, rolling_shutter=0.0)
    assert plain.rolling_shutter == zero.rolling_shutter == 0.0
    a, b = plain.run_video(clips[fmt], chunk=CHUNK, pixel_format=fmt), zero.run_video(clips[fmt], chunk=CHUNK, pixel_format=fmt)
    assert torch.equal(a, b) and zero.shutter_rates is None and plain.shutter_rates is None
    assert torch.equal(_bits(zero.smooth_correction), _bits(plain.smooth_correction))
    # a call that corrected leaves nothing behind for one that does not
    vs = VideoStabilizer(net, batch=8, smooth=SIGMA, rolling_shutter=R)
    c = vs.run_video(clips[fmt], chunk=CHUNK, pixel_format=fmt)
    assert vs.shutter_rates is not None and not torch.equal(c, a)   # (a real correction on this clip)
    vs.rolling_shutter = 0.0
    assert torch.equal(vs.run_video(clips[fmt], chunk=CHUNK, pixel_format=fmt), a) and vs.shutter_rates is None


def _by_hand(vs, src, fmt, cuts=None, zoom=None):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    planes = S.window_planes(src) if fmt == "bgr24" else S.window_planes_yuv(src, fmt)
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    half = vs.period // 2
    with torch.no_grad():
        for cs in range(0, T, CHUNK):   # pass 1's generator calls: per chunk, on the chunk's planes and what its windows reach
            ce = min(T, cs + CHUNK)
            hl, hr = min(half, cs), min(half, T - ce)
            sc = [t - (cs - hl) for t in (cuts or []) if cs - hl < t < ce + hr] or None
            vs._fields(planes[cs - hl:ce + hr], hl, hr, fields[cs:ce], sc)
    seen = PF.grid_sample(planes.unsqueeze(1), fields, align_corners=vs.align_corners).squeeze(1)
    motion, _ = S.global_motion(seen, pixel_scale=(W / 256.0, H / 256.0))
    d, _ = S.smooth_path(motion, vs.smooth, scene_cuts=cuts)
    rates = S.shutter_rates(motion, scene_cuts=cuts)
    kw = dict(align_corners=vs.align_corners, mode=vs.interpolation)
    comp, unc = PF.compose_fields(fields, d, (H, W), return_uncovered=True, rates=rates, rolling_shutter=vs.rolling_shutter, **kw)
    if zoom == "auto":
        bounds = S.field_homography(comp, (H, W))[1]
        window = S.zoom_window(S.auto_crop_window(bounds, (H, W), None, vs.period, scene_cuts=cuts), (H, W))
        assert vs.zoom_windows == [window] * T
        comp = PF.zoom_fields(comp, window, (H, W), **kw)
    out = PF.warp(src, comp, PF.frame_format(fmt, src, "test"), swap_rb=vs.swap_rb, **kw)
    return out, {"smooth_motion": motion, "smooth_correction": d, "shutter_rates": rates, "smooth_uncovered": unc}


CASES = [("bgr24", {}), ("nv12", {}), ("bgr24", {"scene_cuts": [13]}), ("nv12", {"zoom": "auto"}), ("bgr24", {"zoom": "auto", "scene_cuts": [13], "in_flight": 2})]
IDS = ["%s-%s" % (f, "-".join(sorted(k)) or "plain") for f, k in CASES]


@pytest.mark.parametrize("fmt,call", CASES, ids=IDS)
def test_frames_are_the_by_hand_assembly(hip, net, clips, fmt, call):
    from pwstablenet_amd.stream import VideoStabilizer
    src = clips[fmt]
    vs = VideoStabilizer(net, batch=8, smooth=SIGMA, rolling_shutter=R)
    got = vs.run_video(src, chunk=CHUNK, pixel_format=fmt, **call)
    cuts = call.get("scene_cuts")
    want, pieces = _by_hand(vs, src, fmt, cuts, call.get("zoom"))
    for name, value in pieces.items():
        got_v = getattr(vs, name)
        assert got_v.is_cuda and got_v.dtype == value.dtype and got_v.shape == value.shape and torch.equal(_bits(got_v), _bits(value)), name
    assert tuple(vs.shutter_rates.shape) == (T, 2, 4) and vs.shutter_rates.dtype == torch.float64 and torch.isfinite(vs.shutter_rates).all()
    assert float(vs.shutter_rates[:, :, 2:].abs().max()) > 1.0   # the clip's shake, in frame pixels per frame
    for t in [0] + (cuts or []):    # a scene's first frame has one pair: twice
        assert torch.equal(vs.shutter_rates[t, 0], vs.shutter_rates[t, 1])
    for t in [c - 1 for c in (cuts or [])] + [T - 1]:
        assert torch.equal(vs.shutter_rates[t, 0], vs.shutter_rates[t, 1])
    assert got.shape == want.shape and torch.equal(got, want)


class _Stub:
    """A generator stand-in for the argument checks, which come before any generator call."""

    def __call__(self, x, is_training):
        raise AssertionError("the generator must not run")


def test_arguments_that_cannot_work_are_refused(hip):
    from pwstablenet_amd.stream import VideoStabilizer
    for bad in (1.5, -1.0001, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="rolling_shutter"):
            VideoStabilizer(_Stub(), batch=8, smooth=SIGMA, rolling_shutter=bad)
    for r in (R, -1.0):
        with pytest.raises(ValueError, match="smooth"):
            VideoStabilizer(_Stub(), batch=8, rolling_shutter=r)
        with pytest.raises(ValueError, match="smooth"):
            VideoStabilizer(_Stub(), batch=8, smooth=0.0, rolling_shutter=r)
    assert VideoStabilizer(_Stub(), smooth=SIGMA, rolling_shutter=-1).rolling_shutter == -1.0
    assert VideoStabilizer(_Stub(), rolling_shutter=0).rolling_shutter == 0.0
    frames = torch.zeros((34, H, W, 3), dtype=torch.uint8, device="cuda")
    vs = VideoStabilizer(_Stub(), batch=8, smooth=SIGMA, rolling_shutter=R)
    with pytest.raises(ValueError, match="whole clip"):
        vs.run_video(frames, halo_left=2)
    with pytest.raises(ValueError, match="whole clip"):
        vs.run_video(frames, halo_right=3)
    for borders in ("keep", "mosaic"):
        with pytest.raises(ValueError, match=borders):
            VideoStabilizer(_Stub(), batch=8, smooth=SIGMA, rolling_shutter=R, borders=borders).run_video(frames)
    vs.smooth = 0.0   # (set after construction: the call refuses)
    with pytest.raises(ValueError, match="smooth"):
        vs.run_video(frames)
