"""GPU tests of the L1-optimal path in the streaming stabiliser, VideoStabilizer(smooth="l1"): the frames are those assembled by hand from
the same steps -- kept fields -> grid_sample of the planes -> global_motion in frame pixels -> optimal_path [-> shutter_rates] [-> limit_path]
-> compose_fields -> the format's fused warp -- bit for bit; and an identity generator turns a clip whose shake lies inside the reach into
one whose measured path is static.  tests/test_hip_smooth_stream.py's generator and clips: ngf = 16, 40 frames of 640 x 320, batch 8,
chunk 16."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_hip_smooth_stream as SS  # noqa: E402
from test_hip_smooth_stream import clip, clip_nv12, net  # noqa: E402,F401  (the fixtures)

T, H, W, CHUNK = SS.T, SS.H, SS.W, SS.CHUNK


def _by_hand(vs, src, fmt, cuts=None):
    """The frames from the steps, and the pieces the stabiliser publishes."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    planes = S.window_planes(src) if fmt == "bgr24" else S.window_planes_yuv(src, fmt)
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    half = vs.period // 2
    with torch.no_grad():
        for cs in range(0, T, CHUNK):
            ce = min(T, cs + CHUNK)
            hl, hr = min(half, cs), min(half, T - ce)
            sc = [t - (cs - hl) for t in (cuts or []) if cs - hl < t < ce + hr] or None
            vs._fields(planes[cs - hl:ce + hr], hl, hr, fields[cs:ce], sc)
    seen = PF.grid_sample(planes.unsqueeze(1), fields, align_corners=vs.align_corners).squeeze(1)
    motion, inl = S.global_motion(seen, pixel_scale=(W / 256.0, H / 256.0))
    d, path, info = S.optimal_path(motion, (H, W), vs.l1_reach, vs.l1_weights, scene_cuts=cuts, return_info=True)
    pieces = {"smooth_motion": motion, "smooth_inliers": inl, "smooth_path": path, "smooth_l1_info": info}
    kw = dict(align_corners=vs.align_corners, mode=vs.interpolation)
    rs = vs.rolling_shutter
    rates = S.shutter_rates(motion, scene_cuts=cuts) if rs else None
    if rs:
        pieces["shutter_rates"] = rates
    if vs.max_crop is not None:
        pieces["smooth_correction_unlimited"] = d
        d, pieces["limit_strength"], pieces["limit_need"], pieces["limit_uncovered"] = S.limit_path(
            d, fields, (H, W), 1.0 - vs.max_crop, levels=vs.limit_levels, relax=1.0 / (vs.period // 2), scene_cuts=cuts, rates=rates,
            rolling_shutter=rs, **kw)
    pieces["smooth_correction"] = d
    comp, pieces["smooth_uncovered"] = PF.compose_fields(fields, d, (H, W), return_uncovered=True, rates=rates, rolling_shutter=rs, **kw)
    return PF.warp(src, comp, PF.frame_format(fmt, src, "test"), swap_rb=vs.swap_rb, **kw), pieces


CASES = [("bgr24", 1, {}, {}), ("nv12", 2, {}, {}), ("bgr24", 2, {}, {"scene_cuts": [20]}), ("nv12", 1, {"max_crop": 0.05}, {}),
         ("bgr24", 1, {"rolling_shutter": 0.3}, {})]
IDS = ["%s-%d-%s" % (f, n, "-".join("%s" % v for v in list(c.values()) + list(k.values())) or "plain") for f, n, c, k in CASES]


@pytest.mark.parametrize("fmt,in_flight,ctor,call", CASES, ids=IDS)
def test_frames_are_the_by_hand_assembly(hip, net, clip, clip_nv12, fmt, in_flight, ctor, call):
    from pwstablenet_amd.stream import VideoStabilizer
    src = clip if fmt == "bgr24" else clip_nv12
    vs = VideoStabilizer(net, batch=8, smooth="l1", swap_rb=True, **ctor)
    got = vs.run_video(src, chunk=CHUNK, in_flight=in_flight, pixel_format=fmt, **call)
    cuts = call.get("scene_cuts")
    want, pieces = _by_hand(vs, src, fmt, cuts)
    for name, value in pieces.items():
        got_v = getattr(vs, name)
        assert got_v.is_cuda and SS._same(got_v, value), name
    scenes = 1 + len(cuts or [])
    assert tuple(vs.smooth_l1_info.shape) == (scenes, 4, 4) and tuple(vs.smooth_correction.shape) == (T, 6)
    info = vs.smooth_l1_info.cpu().numpy()
    print("steps %s converged %s" % (info[:, :, 0].tolist(), info[:, :, 3].tolist()))
    assert (info[:, :, 0] <= 64).all() and torch.isfinite(vs.smooth_correction).all()
    ident = torch.tensor([1.0, 0, 0, 0, 1.0, 0], dtype=torch.float64, device="cuda")
    unlimited = vs.smooth_correction_unlimited if vs.max_crop is not None else vs.smooth_correction
    assert float((unlimited - ident).abs().max()) > 0.5   # a real correction
    assert got.shape == want.shape and torch.equal(got, want)
    if not ctor and not call:   # a call with a float smooth leaves no L1 result behind
        vs.smooth = 4.0
        vs.run_video(src, chunk=CHUNK, pixel_format=fmt)
        assert vs.smooth_l1_info is None and vs.smooth_correction is not None


def _still_clip(n, h, w, seed, sigma):
    """tests/test_hip_smooth_stream.py's textured scene without its pan: Gaussian jitter of the pose about one place, (n, h, w, 3) uint8."""
    rs = np.random.RandomState(seed)
    k = 12
    wl, ang, ph = rs.uniform(14.0, 90.0, k), rs.uniform(0, 2 * np.pi, k), rs.uniform(0, 2 * np.pi, k)
    kx, ky = 2 * np.pi / wl * np.cos(ang), 2 * np.pi / wl * np.sin(ang)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    a = kx[:, None, None] * xx + ky[:, None, None] * yy + ph[:, None, None]
    sa, ca = np.sin(a).astype(np.float32).reshape(k, -1), np.cos(a).astype(np.float32).reshape(k, -1)
    tx, ty = rs.normal(0, sigma, n), rs.normal(0, sigma, n)
    phi = kx[None] * tx[:, None] + ky[None] * ty[:, None]
    v = np.cos(phi).astype(np.float32) @ sa + np.sin(phi).astype(np.float32) @ ca
    base = np.clip(np.rint(127.5 + 127.5 * 0.13 * v), 0, 255).reshape(n, h, w).astype(np.float32)
    col = np.stack([base * 0.9, base * 1.0, base * 0.8], -1) + rs.randint(-3, 4, (n, h, w, 3))
    return np.clip(col, 0, 255).astype(np.uint8)


def test_shake_inside_the_reach_comes_out_static(hip):
    """A hand-held "static" shot: jitter of 3 px about one place, 40 frames of 640 x 320, under the identity generator (align_corners=True),
    which makes smooth="l1" a classical stabiliser.  The shake lies inside the reach (0.1 of the frame: 32 px and 16 px), so a static path
    is feasible, its objective is 0, and the solver must find it: the translation path P^ = P + exp(lambda) Rot(theta) (D2, D5) has first
    differences below 1e-6 px, where the Gaussian's only shrink.  The output scores steadier than the input on the repository's own
    metric; the score of smooth=4 on the same clip is printed beside it, not gated."""
    from pwstablenet_amd.lib.networks_cascading import define_G
    from pwstablenet_amd.stream import VideoStabilizer
    g = define_G(31, 2, 16, "normal", 0.02)
    g.load_state_dict(SS._state(identity=True))
    g.module.align_corners = True
    g = g.cuda()
    still = torch.from_numpy(_still_clip(T, H, W, 31, 3.0)).cuda()
    vs = VideoStabilizer(g, batch=8, metrics=True, smooth="l1")
    out = vs.run_video(still, chunk=CHUNK)
    assert out.shape == still.shape
    rep = vs.stability_report()
    s_in, s_out = rep["stability_in"]["stability"], rep["stability_out"]["stability"]
    P, D, info = vs.smooth_path.cpu().numpy(), vs.smooth_correction.cpu().numpy(), vs.smooth_l1_info.cpu().numpy()
    s, c, sn = np.exp(P[:, 0]), np.cos(P[:, 1]), np.sin(P[:, 1])
    px, py = P[:, 2] + s * (c * D[:, 2] - sn * D[:, 5]), P[:, 3] + s * (sn * D[:, 2] + c * D[:, 5])
    step = max(float(np.abs(np.diff(px)).max()), float(np.abs(np.diff(py)).max()))
    gauss = VideoStabilizer(g, batch=8, metrics=True, smooth=4.0)
    gauss.run_video(still, chunk=CHUNK)
    s_gauss = gauss.stability_report()["stability_out"]["stability"]
    print("stability in %.4f, out %.4f under \"l1\", %.4f under smooth=4; measured path range x %.2f y %.2f px; largest step of P^ %.3g px; "
          "steps %s converged %s" % (s_in, s_out, s_gauss, np.ptp(P[:, 2]), np.ptp(P[:, 3]), step, info[0, :, 0].tolist(), info[0, :, 3].tolist()))
    assert rep["unfit_pairs_in"] == rep["unfit_pairs_out"] == 0
    assert np.ptp(P[:, 2]) <= 2 * 32.0 and np.ptp(P[:, 3]) <= 2 * 16.0   # the premise: a static path fits the box
    assert step < 1e-6
    assert s_out > s_in
