"""GPU tests of path smoothing in the streaming stabiliser, VideoStabilizer(smooth=sigma): smooth=0 is the stabiliser without the argument
bit for bit; with smooth=4 the frames are those assembled by hand from the same steps -- kept fields -> grid_sample of the planes ->
global_motion in frame pixels -> smooth_path -> compose_fields -> the format's fused warp -- bit for bit, in every mode; and an identity
generator turns a shaky textured clip into one that the repository's own metric scores steadier, past a gate taken from the CPU
restatement of the same chain.  ngf=16 generator as in tests/test_hip_motion_stream.py, 40 frames of 640 x 320, batch 8, chunk 16."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":   # (run as a script it prints the CPU chain's scores; under pytest the conftest has the root on the path)
    sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pwstablenet_amd import synth  # noqa: E402

T, H, W = 40, 320, 640
SIGMA = 4.0
CHUNK = 16
ATTRS = ("smooth_motion", "smooth_inliers", "smooth_path", "smooth_correction", "smooth_uncovered")
# the CPU restatement of test (c)'s chain on test (c)'s clip (cpu_chain below; `python tests/test_hip_smooth_stream.py` prints them)
CPU_STABILITY_IN, CPU_STABILITY_OUT = 0.2730, 0.7293
GATE = math.sqrt(CPU_STABILITY_IN * CPU_STABILITY_OUT)   # 0.4462


def _state(identity=False):
    sd = {"module." + k: torch.from_numpy(v.copy()) for k, v in synth.make_weights("W1", seed=123, ngf=16)}
    if identity:   # the head's bias at identity and nothing else feeding the field: affine_grid(identity) + tanh(tanh(0))
        sd["module.linear.mpconv.0.weight"].zero_()
        sd["module.linear.mpconv.0.bias"].copy_(torch.from_numpy(synth.IDENTITY_THETA))
        sd["module.out.mpconv.0.weight"].zero_()
        sd["module.out.mpconv.0.bias"].zero_()
    return sd


@pytest.fixture(scope="module")
def net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    g = define_G(31, 2, 16, "normal", 0.02)
    g.load_state_dict(_state())
    return g.cuda()


def _texture_u8(n, h, w, seed, lam=(14.0, 90.0), sigma=3.0):
    """tests/test_hip_motion_stream.py's shaky textured scene, (n, h, w) uint8: twelve sinusoids under a pan of (1.0, 0.4) pixel a frame plus
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


def _clip_u8(n, h, w, seed, **kw):
    rs = np.random.RandomState(seed)
    base = _texture_u8(n, h, w, seed, **kw).astype(np.float32)
    col = np.stack([base * 0.9, base * 1.0, base * 0.8], -1) + rs.randint(-3, 4, (n, h, w, 3))
    return np.clip(col, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def clip():
    return torch.from_numpy(_clip_u8(T, H, W, 21)).cuda()


@pytest.fixture(scope="module")
def clip_nv12():
    y = _texture_u8(T, H, W, 22)
    uv = synth.smooth_frames_u8(1, T, H // 2, W, 23)[0] // 2 + 64
    return torch.from_numpy(np.concatenate([y, uv], 1)).cuda()


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def test_smooth_zero_is_the_stabiliser_without_the_argument(hip, net, clip):
    from pwstablenet_amd.stream import VideoStabilizer
    plain = VideoStabilizer(net, batch=8)
    zero = VideoStabilizer(net, batch=8, smooth=0.0)
    assert plain.smooth == zero.smooth == 0.0
    for kw in ({}, {"crop": "auto"}, {"zoom": "auto", "in_flight": 2}):
        assert torch.equal(zero.run_video(clip, chunk=16, **kw), plain.run_video(clip, chunk=16, **kw))
        assert all(getattr(zero, a) is None for a in ATTRS) and all(getattr(plain, a) is None for a in ATTRS)
    # a call that smoothed leaves nothing behind for one that does not
    vs = VideoStabilizer(net, batch=8, smooth=SIGMA)
    vs.run_video(clip, chunk=16)
    assert all(getattr(vs, a) is not None for a in ATTRS)
    vs.smooth = 0.0
    assert torch.equal(vs.run_video(clip, chunk=16), plain.run_video(clip, chunk=16)) and all(getattr(vs, a) is None for a in ATTRS)


def _by_hand(vs, src, fmt, cuts=None, crop=None, zoom=None):
    """The frames from the steps, and the pieces the stabiliser publishes."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    planes = S.window_planes(src) if fmt == "bgr24" else S.window_planes_yuv(src, fmt)
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    half = vs.period // 2
    with torch.no_grad():
        for cs in range(0, T, CHUNK):   # pass 1's generator calls: per chunk, on the chunk's planes and what its windows reach, batches restarting at a cut
            ce = min(T, cs + CHUNK)
            hl, hr = min(half, cs), min(half, T - ce)
            sc = [t - (cs - hl) for t in (cuts or []) if cs - hl < t < ce + hr] or None
            vs._fields(planes[cs - hl:ce + hr], hl, hr, fields[cs:ce], sc)
    if vs.rigidity > 0:
        fields = PF.rigid_fields(fields, S.field_homography(fields, (H, W))[0], (H, W), vs.rigidity)
    seen = PF.grid_sample(planes.unsqueeze(1), fields, align_corners=vs.align_corners).squeeze(1)
    motion, inl = S.global_motion(seen, pixel_scale=(W / 256.0, H / 256.0))
    d, path = S.smooth_path(motion, vs.smooth, scene_cuts=cuts)
    kw = dict(align_corners=vs.align_corners, mode=vs.interpolation)
    comp, unc = PF.compose_fields(fields, vs.smooth_correction, (H, W), return_uncovered=True, **kw)
    bounds = S.field_homography(comp, (H, W))[1]
    if zoom == "auto":
        window = S.zoom_window(S.auto_crop_window(bounds, (H, W), None, vs.period, scene_cuts=cuts), (H, W))
        assert vs.zoom_windows == [window] * T
        comp = PF.zoom_fields(comp, window, (H, W), **kw)
    elif zoom is not None:   # a fraction: the one centred window, which smoothing moves from the single pass into pass 2
        assert vs.zoom_windows == [(0.5 * W - 0.5 * zoom * W, 0.5 * W + 0.5 * zoom * W, 0.5 * H - 0.5 * zoom * H, 0.5 * H + 0.5 * zoom * H)] * T
        comp = PF.zoom_fields(comp, vs.zoom_windows[0], (H, W), **kw)
    out = PF.warp(src, comp, PF.frame_format(fmt, src, "test"), swap_rb=vs.swap_rb, **kw)
    if vs.edge != "pad":
        PF.edge_borders_(out, src, comp, vs.edge, fmt, swap_rb=vs.swap_rb, **kw)
    if crop == "auto":
        c = S.auto_crop_window(bounds, (H, W), (H, W), vs.period, scene_cuts=cuts)
        out = out[:, int(c[2]):int(c[3]), int(c[0]):int(c[1])]
        assert out.shape[1] < H or out.shape[2] < W   # a real crop on this clip
    return out, {"smooth_motion": motion, "smooth_inliers": inl, "smooth_path": path, "smooth_correction": d, "smooth_uncovered": unc}, bounds


CASES = [("bgr24", 1, {}, {}), ("bgr24", 2, {}, {}), ("nv12", 1, {}, {}), ("nv12", 2, {}, {}),
         ("bgr24", 1, {}, {"crop": "auto"}), ("bgr24", 2, {}, {"zoom": "auto"}), ("bgr24", 1, {"edge": "mirror"}, {}),
         ("nv12", 1, {"rigidity": 0.5}, {}), ("bgr24", 2, {}, {"scene_cuts": [20]}), ("nv12", 2, {}, {"zoom": 0.9})]
IDS = ["%s-%d-%s" % (f, n, "-".join("%s" % v for v in list(c.values()) + list(k.values())) or "plain") for f, n, c, k in CASES]


@pytest.mark.parametrize("fmt,in_flight,ctor,call", CASES, ids=IDS)
def test_frames_are_the_by_hand_assembly(hip, net, clip, clip_nv12, fmt, in_flight, ctor, call):
    from pwstablenet_amd.stream import VideoStabilizer
    src = clip if fmt == "bgr24" else clip_nv12
    vs = VideoStabilizer(net, batch=8, smooth=SIGMA, swap_rb=True, metrics=True, **ctor)
    got = vs.run_video(src, chunk=16, in_flight=in_flight, pixel_format=fmt, **call)
    cuts = call.get("scene_cuts")
    want, pieces, bounds = _by_hand(vs, src, fmt, cuts, call.get("crop"), call.get("zoom"))
    for name, value in pieces.items():
        got_v = getattr(vs, name)
        assert got_v.is_cuda and _same(got_v, value), name
    assert tuple(vs.smooth_motion.shape) == (T, 4) and tuple(vs.smooth_correction.shape) == (T, 6) and vs.smooth_inliers.dtype == torch.int32
    assert torch.isfinite(vs.smooth_correction).all() and int(vs.smooth_inliers[1:].min()) >= 8
    assert float((vs.smooth_correction - torch.tensor([1.0, 0, 0, 0, 1.0, 0], dtype=torch.float64, device="cuda")).abs().max()) > 0.5   # a real correction
    assert got.shape == want.shape and torch.equal(got, want)
    ident = torch.tensor([1.0, 0, 0, 0, 1.0, 0], dtype=torch.float64, device="cuda")
    for t in [0] + (cuts or []):   # a scene's first frame is on its own smooth path: the odd reflection
        assert float((vs.smooth_correction[t] - ident).abs().max()) <= 1e-9
    # the report describes the field that warps: its bounds are the composed fields'
    rep = vs.stability_report()
    b = bounds.to("cpu", torch.float64).numpy()
    area = np.clip(np.minimum(b[:, 1], H) - np.maximum(b[:, 0], 0), 0, None) * np.clip(np.minimum(b[:, 3], W) - np.maximum(b[:, 2], 0), 0, None) / (H * W)
    assert np.allclose(rep["cropping"]["per_frame"], area, rtol=0, atol=1e-12)
    if not ctor and not call and in_flight == 1:   # host input, metrics off: the same frames
        again = VideoStabilizer(net, batch=8, smooth=SIGMA, swap_rb=True)
        assert torch.equal(again.run_video(src.cpu().pin_memory(), chunk=16, pixel_format=fmt).cuda(), want)


def cpu_chain():
    """Test (c)'s chain in float64 on the CPU -- tests/path_ref.py plus torch's CPU grid_sample: the window planes of the clip (the oracle's
    gray + INTER_AREA), stability in; the identity field under align_corners=True leaves the planes as they are, so the motion the fields
    leave is the planes' own, fitted in frame pixels; path and corrections; the identity field composed with them; the frames warped by the
    composed field resized to the frame (bilinear, zero padding, truncated to bytes); their planes, stability out."""
    import torch.nn.functional as F
    from oracle import frameio_ref

    import motion_ref as R
    import path_ref as P
    clip = _clip_u8(T, H, W, 21)
    planes = np.stack([frameio_ref.window_plane(f, 256) for f in clip])
    s_in = R.stability_scores(R.global_motion(planes)[0])["stability"]
    motion, _ = P.global_motion_scaled(planes, (W / 256.0, H / 256.0))
    _, D = P.path_smooth(motion, SIGMA)
    u, v = np.meshgrid(np.linspace(-1, 1, 256), np.linspace(-1, 1, 256))
    field = np.stack([np.stack([u, v], -1)] * T)
    comp = torch.from_numpy(P.compose64(field, D, (H, W)))
    grid = F.interpolate(comp.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    out = F.grid_sample(torch.from_numpy(clip).permute(0, 3, 1, 2).double(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    out = out.permute(0, 2, 3, 1).clamp(0, 255).floor().to(torch.uint8).numpy()
    planes_out = np.stack([frameio_ref.window_plane(f, 256) for f in out])
    return s_in, R.stability_scores(R.global_motion(planes_out)[0])["stability"]


def test_a_shaky_clip_comes_out_steadier(hip, clip):
    """An identity generator (tests/test_hip_motion_stream.py's, under align_corners=True) makes smooth=4 a classical stabiliser: the shaky
    textured clip must score above the gate, and score below it going in.  The gate is the geometric mean of the two scores the CPU
    restatement of the chain gives on this clip (cpu_chain): stability 0.2730 in, 0.7293 out, gate 0.4462.  Without the feature the
    identity generator returns the clip, and out = in."""
    from pwstablenet_amd.lib.networks_cascading import define_G
    from pwstablenet_amd.stream import VideoStabilizer
    g = define_G(31, 2, 16, "normal", 0.02)
    g.load_state_dict(_state(identity=True))
    g.module.align_corners = True
    vs = VideoStabilizer(g.cuda(), batch=8, metrics=True, smooth=SIGMA)
    out = vs.run_video(clip, chunk=16)
    assert out.shape == clip.shape
    rep = vs.stability_report()
    s_in, s_out = rep["stability_in"]["stability"], rep["stability_out"]["stability"]
    print("stability in %.4f (CPU %.4f), out %.4f (CPU %.4f), gate %.4f; uncovered nodes per frame up to %d"
          % (s_in, CPU_STABILITY_IN, s_out, CPU_STABILITY_OUT, GATE, int(vs.smooth_uncovered.max())))
    assert rep["unfit_pairs_in"] == rep["unfit_pairs_out"] == 0
    assert s_in < GATE < s_out


class _Stub:
    """A generator stand-in for the argument checks, which come before any generator call."""

    def __call__(self, x, is_training):
        raise AssertionError("the generator must not run")


def test_smooth_errors_and_small_frames(hip, net):
    from pwstablenet_amd.stream import VideoStabilizer
    for bad in (-1.0, 256.5, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="sigma"):
            VideoStabilizer(_Stub(), batch=8, smooth=bad)
    assert VideoStabilizer(_Stub(), smooth=256).smooth == 256.0
    frames = torch.zeros((34, H, W, 3), dtype=torch.uint8, device="cuda")
    vs = VideoStabilizer(_Stub(), batch=8, smooth=SIGMA)
    with pytest.raises(ValueError, match="whole clip"):
        vs.run_video(frames, halo_left=2)
    with pytest.raises(ValueError, match="whole clip"):
        vs.run_video(frames, halo_right=3)
    for borders in ("keep", "mosaic"):
        with pytest.raises(ValueError, match=borders):
            VideoStabilizer(_Stub(), batch=8, smooth=SIGMA, borders=borders).run_video(frames)
    # below the fit's 600 x 300 lattice the path is smoothed all the same; nothing is fitted, the report has no cropping
    small = torch.from_numpy(_clip_u8(T, 288, 320, 5, lam=(8.0, 50.0), sigma=2.0)).cuda()
    vs = VideoStabilizer(net, batch=8, smooth=SIGMA, metrics=True)
    out = vs.run_video(small, chunk=16)
    assert out.shape == small.shape and tuple(vs.smooth_correction.shape) == (T, 6) and torch.isfinite(vs.smooth_correction).all()
    assert vs.stability_report()["cropping"] is None
    with pytest.raises(ValueError, match="600 x 300"):
        vs.run_video(small, chunk=16, crop="auto")


if __name__ == "__main__":
    print("stability in %.4f, out %.4f" % cpu_chain())
