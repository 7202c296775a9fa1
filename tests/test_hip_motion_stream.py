"""GPU tests of VideoStabilizer / run_video(metrics=True): the frames are those of metrics=False bit for bit in every mode, motion_in and
motion_out are global_motion of the planes of the input and of the returned frames, scene cuts split the report, and stability_report()
holds what it documents.  ngf=16 generator as in tests/test_hip_scene_cuts.py, 40 frames of 640 x 320."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pwstablenet_amd import synth  # noqa: E402

T, H, W = 40, 320, 640
ATTRS = ("motion_in", "motion_out", "motion_inliers_in", "motion_inliers_out")


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
    """A shaky textured scene, (n, h, w) uint8: twelve sinusoids under a pan of (1.0, 0.4) pixel a frame plus Gaussian jitter of the pose.
    Translations only, so a frame is one small matrix product over the sinusoids' sines and cosines.  (synth.smooth_frames_u8 is too
    smooth for this feature: its blocks stay below global_motion's activity threshold and every pair comes out NaN.)"""
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
    """BGR frames of the textured scene, with a little sensor noise"""
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


def _check_attrs(vs, on):
    for a in ATTRS:
        v = getattr(vs, a)
        if not on:
            assert v is None, a
        else:
            assert v.is_cuda and v.shape == ((T, 4) if "inliers" not in a else (T,))
            assert v.dtype == (torch.float64 if "inliers" not in a else torch.int32)


CASES = [("bgr24", 1, {}, {}), ("bgr24", 2, {}, {}), ("nv12", 1, {}, {}), ("nv12", 2, {}, {}),
         ("bgr24", 1, {"borders": "mosaic"}, {}), ("bgr24", 2, {"edge": "mirror"}, {}), ("nv12", 1, {}, {"zoom": 0.9}),
         ("bgr24", 2, {"rigidity": 0.5}, {"half_size_output": True})]


@pytest.mark.parametrize("fmt,in_flight,ctor,call", CASES)
def test_frames_are_those_without_metrics(hip, net, clip, clip_nv12, fmt, in_flight, ctor, call):
    from pwstablenet_amd.stream import VideoStabilizer
    src = clip if fmt == "bgr24" else clip_nv12
    vs = VideoStabilizer(net, batch=8, **ctor)
    kw = dict(chunk=16, in_flight=in_flight, pixel_format=fmt, **call)
    got = vs.run_video(src, metrics=True, **kw)
    _check_attrs(vs, True)
    rep = vs.stability_report()
    assert rep["cropping"] is not None and len(rep["distortion"]["per_frame"]) == T
    want = vs.run_video(src, metrics=False, **kw)
    _check_attrs(vs, False)
    assert torch.equal(got, want)
    with pytest.raises(RuntimeError, match="metrics=True"):
        vs.stability_report()
    again = VideoStabilizer(net, batch=8, metrics=True, **ctor)   # the constructor's switch is the call's default
    assert torch.equal(again.run_video(src.cpu().pin_memory(), **kw).cuda(), want)
    _check_attrs(again, True)
    plain = VideoStabilizer(net, batch=8, **ctor)
    assert torch.equal(plain.run_video(src, **kw), want)
    _check_attrs(plain, False)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                                                     b.view(torch.int64) if b.dtype == torch.float64 else b)


@pytest.mark.parametrize("fmt,swap_rb,in_flight", [("bgr24", False, 1), ("bgr24", True, 2), ("nv12", False, 1)])
def test_motion_is_global_motion_of_the_input_and_of_the_returned_frames(hip, net, clip, clip_nv12, fmt, swap_rb, in_flight):
    from pwstablenet_amd.stream import VideoStabilizer, global_motion, window_planes, window_planes_yuv
    src = clip if fmt == "bgr24" else clip_nv12
    vs = VideoStabilizer(net, batch=8, swap_rb=swap_rb, metrics=True)
    out = vs.run_video(src, chunk=16, in_flight=in_flight, pixel_format=fmt)

    def planes(x, rgb):
        return window_planes(x, frames_are_rgb=rgb) if fmt == "bgr24" else window_planes_yuv(x, fmt)
    m_in, i_in = global_motion(planes(src, False))
    assert _same(vs.motion_in, m_in) and _same(vs.motion_inliers_in, i_in)
    m_out, i_out = global_motion(planes(out, swap_rb))   # (swap_rb: the returned frames are RGB)
    assert _same(vs.motion_out, m_out) and _same(vs.motion_inliers_out, i_out)
    assert not _same(m_in, m_out)
    assert torch.isfinite(m_in).all() and int(i_in[1:].min()) >= 8   # (the texture is busy enough for the default threshold)
    # a shard reports its own T frames
    shard = vs.run_video(src, chunk=16, halo_left=5, halo_right=7, pixel_format=fmt)
    assert vs.motion_in.shape == (T - 12, 4) and vs.motion_out.shape == (T - 12, 4) and shard.shape[0] == T - 12
    assert _same(vs.motion_in, global_motion(planes(src[5:T - 7].contiguous(), False))[0])
    assert _same(vs.motion_out, global_motion(planes(shard, swap_rb))[0])


def test_scene_cuts_split_the_report_and_metrics_off_resets(hip, net, clip):
    from pwstablenet_amd.stream import VideoStabilizer, stability_scores
    two = torch.cat([clip[:20], torch.from_numpy(_clip_u8(20, H, W, 77) // 2).cuda()])   # (a darker scene: a cut the detector sees)
    vs = VideoStabilizer(net, batch=8, metrics=True)
    vs.run_video(two, chunk=16, scene_cuts=[20])
    rep = vs.stability_report()
    for side in ("in", "out"):
        scenes = rep["stability_" + side]["scenes"]
        assert [(s["start"], s["end"]) for s in scenes] == [(0, 20), (20, 40)]
        assert all(math.isnan(s["stability"]) for s in scenes)   # (20 frames: fewer than the 24 a score needs)
    m = vs.motion_in.cpu().numpy()
    unfit = np.isnan(m).any(1)
    assert rep["unfit_pairs_in"] == int(unfit.sum()) - int(unfit[20])   # pair 20 belongs to neither scene
    # 48 frames, a cut at 24: both scenes have a score, and they are those of the scenes' own rows -- row 24 is not read
    three = torch.cat([clip[:24], torch.from_numpy(_clip_u8(24, H, W, 78)).cuda()])
    vs.run_video(three, chunk=16, scene_cuts=[24], in_flight=2)
    rep = vs.stability_report()
    m = vs.motion_in.cpu().numpy()
    a, b = stability_scores(m[:24]), stability_scores(m[24:])
    got = rep["stability_in"]["scenes"]
    assert got[0]["stability"] == a["stability"] and got[1]["stability"] == b["stability"] and 0.0 < a["stability"] <= 1.0
    assert abs(rep["stability_in"]["stability"] - 0.5 * (a["stability"] + b["stability"])) < 1e-15
    poisoned = m.copy()
    poisoned[24] = np.nan
    assert stability_scores(poisoned, [24])["stability"] == rep["stability_in"]["stability"]
    vs.run_video(two, chunk=16, metrics=False)
    _check_attrs(vs, False)
    auto = VideoStabilizer(net, batch=8, metrics=True)
    auto.run_video(two, chunk=16, scene_cuts="auto")
    assert auto.scene_cuts == [20] and [(s["start"], s["end"]) for s in auto.stability_report()["stability_out"]["scenes"]] == [(0, 20), (20, 40)]


def test_report_keys_and_small_frames(hip, net, clip):
    from pwstablenet_amd.stream import VideoStabilizer
    vs = VideoStabilizer(net, batch=8, metrics=True)
    vs.run_video(clip, chunk=16, crop="auto", half_size_output=True)   # (a two-pass path: its own fit serves the report)
    rep = vs.stability_report()
    assert set(rep) == {"stability_in", "stability_out", "cropping", "distortion", "unfit_pairs_in", "unfit_pairs_out"}
    for side in ("stability_in", "stability_out"):
        assert set(rep[side]) == {"stability", "translation", "rotation", "scenes"}
        assert set(rep[side]["scenes"][0]) == {"start", "end", "translation", "rotation", "stability"}
        assert 0.0 < rep[side]["stability"] <= 1.0 and rep[side]["stability"] == min(rep[side]["translation"], rep[side]["rotation"])
    for key in ("cropping", "distortion"):
        v = rep[key]
        assert set(v) == {"per_frame", "mean", "min"} and len(v["per_frame"]) == T
        assert 0.0 < v["min"] <= v["mean"] <= 1.0 and abs(v["mean"] - float(np.mean(v["per_frame"]))) < 1e-12
    assert rep["unfit_pairs_in"] == 0 and rep["unfit_pairs_out"] >= 0
    # below the fit's 600 x 300 lattice: no cropping and no distortion, stability as ever.  (320 x 288, not the 320 x 240 one might try: the
    # window planes are an INTER_AREA down-scale to 256 x 256 and refuse a smaller source.)
    small = torch.from_numpy(_clip_u8(T, 288, 320, 5, lam=(8.0, 50.0), sigma=2.0)).cuda()
    vs.run_video(small, chunk=16)
    rep = vs.stability_report()
    assert rep["cropping"] is None and rep["distortion"] is None
    assert 0.0 < rep["stability_in"]["stability"] <= 1.0 and 0.0 < rep["stability_out"]["stability"] <= 1.0


def test_identity_field_changes_nothing(hip, clip):
    """The weights synth gives with the head's bias at identity and a silent field head, under the align_corners=True convention, in which
    node j of the identity grid is exactly the pixel the resized field's node sits on: the warp samples every pixel at its own centre and
    every frame's homography is the identity: distortion 1 within 1e-6, nothing cropped.
    The returned frames are the input up to ONE level: the warp's fp32 coordinates land an ulp beside a pixel centre, and the blend of two
    neighbours is truncated to uint8 (measured: 26 % of the bytes are one level lower, none differs by more).  So stability_out equals
    stability_in up to what one level does to the sub-pixel vectors, not to the bit.  The bound is reasoned, not fitted: one level in some of
    a block's 256 samples moves S by at most a few hundred against a parabola curvature of several thousand -- a few hundredths of a pixel
    per block, with either sign; over 196 blocks that is about 0.004 pixel per pair, over the 39 pairs of the path about 0.025 pixel against
    a path that swings by 3 pixels and more: 1 % of its amplitude, 2 % of its energy, on either side of the ratio.  Allowed: 0.02.
    Measured: 3.4e-4 (0.27305 in, 0.27271 out)."""
    from pwstablenet_amd.lib.networks_cascading import define_G
    from pwstablenet_amd.stream import VideoStabilizer
    g = define_G(31, 2, 16, "normal", 0.02)
    g.load_state_dict(_state(identity=True))
    g.module.align_corners = True
    vs = VideoStabilizer(g.cuda(), batch=8, metrics=True)
    out = vs.run_video(clip, chunk=16)
    diff = (out.to(torch.int16) - clip.to(torch.int16)).abs()
    print("identity warp: largest byte difference", int(diff.max()), "bytes that differ", int((diff > 0).sum()), "of", diff.numel())
    assert int(diff.max()) <= 1
    rep = vs.stability_report()
    d, c = np.array(rep["distortion"]["per_frame"]), np.array(rep["cropping"]["per_frame"])
    print("distortion - 1", np.abs(d - 1).max(), "cropping", c.min(), c.max())
    assert np.abs(d - 1.0).max() <= 1e-6   # (measured: 8.4e-9)
    # field_homography's bounds carry no half-pixel term and read this convention's identity as the frame less a pixel or two at each rim
    # (measured: 0.98737 of the frame); within two pixels of every rim is asked for
    assert (H - 4) * (W - 4) / float(H * W) <= c.min() and c.max() <= 1.0
    print("stability in / out", rep["stability_in"], rep["stability_out"])
    assert _same(vs.motion_inliers_in, vs.motion_inliers_out) and rep["unfit_pairs_in"] == rep["unfit_pairs_out"] == 0
    assert float((vs.motion_in - vs.motion_out).abs().max()) <= 0.05
    # (the clip does not rotate: its rotation signal is the estimator's own noise, 1e-5 rad, and one level changes it as much as it is --
    # measured 0.812 in, 0.860 out; it is not the smaller part and is not compared)
    assert rep["stability_in"]["stability"] == rep["stability_in"]["translation"]
    for key in ("stability", "translation"):
        assert abs(rep["stability_out"][key] - rep["stability_in"][key]) <= 0.02, key
