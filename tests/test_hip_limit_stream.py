"""GPU tests of crop-bounded smoothing in the streaming stabiliser, VideoStabilizer(smooth=sigma, max_crop=c): max_crop=None and a budget
that never binds are today's smooth=sigma bit for bit; with a budget that binds the protected window shows no wedge, the strengths and
levels lie inside the float64 restatement's bounds (tests/limit_ref.py), the frames are those assembled by hand from the steps --
limit_path between smooth_path and compose_fields -- and the clip still comes out steadier than a gate taken from the CPU chain.
Identity generator under align_corners=True (tests/test_hip_smooth_stream.py's), 40 frames of 640 x 320, smooth=4, batch 8, chunk 16.

The CPU chain on this clip (`python tests/test_hip_limit_stream.py` prints it; cpu_chain below), float64, on the path measured from the
window planes, k = 0.97 (margins 9.6 x 4.8 pixels), 16 levels, relax 1/12:
  the unlimited corrections reach 5.51 px in x and 9.16 px in y; under them 12 of 40 frames leave nodes of the window's rectangle (nodes
  3 .. 252 on both axes) uncovered (at least 5 are asked for), up to 1250 nodes; those 12 frames need limiting (need < 16), the smallest
  need is 6 of 16 (strength 0.375); at 1/12 per frame the limited frames lie so close together that after the sweeps all 40 frames lie
  below 1 (the largest strength is 0.979), the mean strength is 0.695; no node of the rectangle is uncovered under the limited
  corrections; stability 0.2730 in, 0.7293 out unlimited, 0.3550 out limited -- on this clip, whose shake exceeds the 4.8-pixel budget
  in y on a third of the frames, the budget costs most of the gain: the gate is sqrt(0.2730 x 0.3550) = 0.3113.
On an MI355X the device reports the same 40 levels as this chain, stability 0.2730 in and 0.3549 out; zoom=0.97's own count on the zoomed
field's nodes -- the window itself, not the cells around it -- finds wedges on 8 frames of the unlimited run (up to 1024 nodes) and on none
of the limited one."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":   # (run as a script it prints the CPU chain's figures; under pytest the conftest has the root on the path)
    sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pwstablenet_amd import synth  # noqa: E402

T, H, W = 40, 320, 640
SIGMA = 4.0
CHUNK = 16
CROP = 0.03
K = 1.0 - CROP
LEVELS = 16
RELAX = 1.0 / 12   # 1 / ceil(3 sigma)
LIMIT_ATTRS = ("limit_strength", "limit_need", "limit_uncovered", "smooth_correction_unlimited")
CPU_STABILITY_IN, CPU_STABILITY_OUT_LIMITED = 0.2730, 0.3550
GATE = math.sqrt(CPU_STABILITY_IN * CPU_STABILITY_OUT_LIMITED)


def _state():
    """tests/test_hip_smooth_stream.py's identity generator: the head's bias at identity and nothing else feeding the field."""
    sd = {"module." + k: torch.from_numpy(v.copy()) for k, v in synth.make_weights("W1", seed=123, ngf=16)}
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


def _kept_fields(vs, planes, cuts=None):
    """pass 1's generator calls: per chunk, on the chunk's planes and what its windows reach, batches restarting at a cut"""
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    half = vs.period // 2
    with torch.no_grad():
        for cs in range(0, T, CHUNK):
            ce = min(T, cs + CHUNK)
            hl, hr = min(half, cs), min(half, T - ce)
            sc = [t - (cs - hl) for t in (cuts or []) if cs - hl < t < ce + hr] or None
            vs._fields(planes[cs - hl:ce + hr], hl, hr, fields[cs:ce], sc)
    return fields


def test_no_budget_and_a_budget_that_never_binds_are_todays_smoothing(hip, net, clip):
    from pwstablenet_amd.stream import VideoStabilizer
    today = VideoStabilizer(net, batch=8, smooth=SIGMA)
    want = today.run_video(clip, chunk=CHUNK)
    assert today.max_crop is None and all(getattr(today, a) is None for a in LIMIT_ATTRS)
    none = VideoStabilizer(net, batch=8, smooth=SIGMA, max_crop=None)
    assert torch.equal(none.run_video(clip, chunk=CHUNK), want) and all(getattr(none, a) is None for a in LIMIT_ATTRS)
    half = VideoStabilizer(net, batch=8, smooth=SIGMA, max_crop=0.5)
    assert torch.equal(half.run_video(clip, chunk=CHUNK), want)
    assert half.limit_strength.dtype == torch.float64 and tuple(half.limit_strength.shape) == (T,) and bool((half.limit_strength == 1.0).all())
    assert bool((half.limit_need == half.limit_levels).all()) and bool((half.limit_uncovered == 0).all())
    assert _same(half.smooth_correction, today.smooth_correction) and _same(half.smooth_correction_unlimited, today.smooth_correction)
    # a call that limited leaves nothing behind for one that does not
    half.max_crop = None
    assert torch.equal(half.run_video(clip, chunk=CHUNK), want) and all(getattr(half, a) is None for a in LIMIT_ATTRS)


def test_a_binding_budget_keeps_the_window_covered(hip, net, clip):
    """zoom=0.97 shows wedges on several frames of the unlimited run and on none of the limited one; the levels and strengths lie inside the
    float64 restatement's bounds on the same measured corrections and the same fields."""
    import limit_ref as L
    from pwstablenet_amd import stream as S
    from pwstablenet_amd.stream import VideoStabilizer
    free = VideoStabilizer(net, batch=8, smooth=SIGMA)
    free.run_video(clip, chunk=CHUNK, zoom=K)
    wedged = int((free.zoom_uncovered > 0).sum())
    vs = VideoStabilizer(net, batch=8, smooth=SIGMA, max_crop=CROP)
    assert vs.limit_levels == LEVELS and vs.limit_relax is None
    out = vs.run_video(clip, chunk=CHUNK, zoom=K)
    assert out.shape == clip.shape
    strength, need = vs.limit_strength.cpu().numpy(), vs.limit_need.cpu().numpy()
    print("unlimited: %d frames with wedges at zoom %.2f, up to %d nodes; limited: need %s, strength min %.4f mean %.4f, %d below 1"
          % (wedged, K, int(free.zoom_uncovered.max()), need.tolist(), strength.min(), strength.mean(), int((strength < 1).sum())))
    assert wedged >= 5
    assert int(vs.zoom_uncovered.max()) == 0 and int(vs.limit_uncovered.max()) == 0
    assert _same(vs.smooth_correction_unlimited, free.smooth_correction) and vs.limit_need.dtype == torch.int32
    # the restatement on what the device measured: the identity generator's fields and the unlimited corrections
    fields = _kept_fields(vs, S.window_planes(clip)).cpu().numpy()
    d = vs.smooth_correction_unlimited.cpu().numpy()
    rect = L.rectangle(K, (H, W), (256, 256))
    assert rect == S.limit_rectangle(K, (H, W), (256, 256))
    lo, hi, share = L.reach_bounds(fields, d[:, None, :], (H, W), rect, True, 0)   # under the whole correction, every frame
    assert share < 0.01   # (the reference alone)
    bound = np.flatnonzero(lo[:, 0] > 0)
    assert len(bound) >= 5   # the budget binds on several frames, by the reference alone
    # the levels, walked in float64 for the frames that the whole correction leaves uncovered and a few that it does not (the whole
    # clip at every level is a quarter of a minute of numpy)
    frames = bound.tolist() + np.flatnonzero(hi[:, 0] == 0)[::10].tolist()
    need_lo, need_hi = L.need_bounds(fields, d, LEVELS, (H, W), rect, True, 0, frames)
    print("frames %s: float64 need %s .. %s" % (frames, need_lo.tolist(), need_hi.tolist()))
    assert (need_lo <= need[frames]).all() and (need[frames] <= need_hi).all() and need.min() >= 0
    assert (need_hi[:len(bound)] < LEVELS).all() and (need[bound] < LEVELS).all()
    # the strengths: exactly the two sweeps over the levels that the device reported, and inside the sweeps over the reference's bounds
    # (a frame that was not walked: anything from 0 to the whole correction)
    assert strength.tobytes() == L.sweeps(np.maximum(need, 0) / float(LEVELS), RELAX).tobytes()
    pess, opt = np.zeros(T), np.full(T, float(LEVELS))
    pess[frames], opt[frames] = need_lo, need_hi
    s_lo, s_hi = L.sweeps(np.maximum(pess, 0) / LEVELS, RELAX), L.sweeps(np.maximum(opt, 0) / LEVELS, RELAX)
    assert (s_lo <= strength).all() and (strength <= s_hi).all()
    assert int((strength < 1).sum()) >= len(bound) and int((strength == 1).sum()) >= int((s_lo == 1).sum())
    # what was composed is D(strength) of what was measured
    want_d = np.array([d[t] if strength[t] == 1.0 else L.level_row(d[t], strength[t]) for t in range(T)])
    got_d = vs.smooth_correction.cpu().numpy()
    assert (np.abs(got_d - want_d) <= 1e-14 * np.maximum(np.abs(want_d), 1.0)).all()
    assert got_d[strength == 1.0].tobytes() == d[strength == 1.0].tobytes()


def _by_hand(vs, src, fmt, cuts=None, zoom=None):
    """The frames from the steps, and the pieces the stabiliser publishes."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    planes = S.window_planes(src) if fmt == "bgr24" else S.window_planes_yuv(src, fmt)
    fields = _kept_fields(vs, planes, cuts)
    seen = PF.grid_sample(planes.unsqueeze(1), fields, align_corners=vs.align_corners).squeeze(1)
    motion, _ = S.global_motion(seen, pixel_scale=(W / 256.0, H / 256.0))
    d, _ = S.smooth_path(motion, vs.smooth, scene_cuts=cuts)
    kw = dict(align_corners=vs.align_corners, mode=vs.interpolation)
    rates = S.shutter_rates(motion, scene_cuts=cuts) if vs.rolling_shutter else None
    d_lim, strength, need, left = S.limit_path(d, fields, (H, W), 1.0 - vs.max_crop, levels=vs.limit_levels, relax=1.0 / math.ceil(3 * vs.smooth),
                                               scene_cuts=cuts, rates=rates, rolling_shutter=vs.rolling_shutter, **kw)
    comp, unc = PF.compose_fields(fields, d_lim, (H, W), return_uncovered=True, rates=rates, rolling_shutter=vs.rolling_shutter, **kw)
    if zoom is not None:
        comp = PF.zoom_fields(comp, S._centred_window(zoom, H, W), (H, W), **kw)
    out = PF.warp(src, comp, PF.frame_format(fmt, src, "test"), swap_rb=vs.swap_rb, **kw)
    return out, {"smooth_correction_unlimited": d, "smooth_correction": d_lim, "limit_strength": strength, "limit_need": need,
                 "limit_uncovered": left, "smooth_uncovered": unc}


CASES = [("bgr24", 1, {}, {}), ("nv12", 2, {}, {}), ("bgr24", 2, {}, {"scene_cuts": [20]}), ("bgr24", 1, {"rolling_shutter": 0.5}, {}),
         ("nv12", 1, {"rolling_shutter": -0.5, "interpolation": "bicubic"}, {"zoom": K, "scene_cuts": [13]})]
IDS = ["%s-%d-%s" % (f, n, "-".join("%s" % v for v in list(c.values()) + list(k.values())) or "plain") for f, n, c, k in CASES]


@pytest.mark.parametrize("fmt,in_flight,ctor,call", CASES, ids=IDS)
def test_frames_are_the_by_hand_assembly(hip, net, clip, clip_nv12, fmt, in_flight, ctor, call):
    from pwstablenet_amd.stream import VideoStabilizer
    src = clip if fmt == "bgr24" else clip_nv12
    vs = VideoStabilizer(net, batch=8, smooth=SIGMA, max_crop=CROP, **ctor)
    got = vs.run_video(src, chunk=CHUNK, in_flight=in_flight, pixel_format=fmt, **call)
    cuts = call.get("scene_cuts")
    want, pieces = _by_hand(vs, src, fmt, cuts, call.get("zoom"))
    for name, value in pieces.items():
        got_v = getattr(vs, name)
        assert got_v.is_cuda and _same(got_v, value), name
    assert got.shape == want.shape and torch.equal(got, want)
    strength = vs.limit_strength.cpu().numpy()
    assert int((strength < 1).sum()) >= 1   # a budget that binds
    for a, b in zip([0] + (cuts or []), (cuts or []) + [T]):   # eased inside a scene, free to jump at a cut
        assert (np.abs(np.diff(strength[a:b])) <= 1.0 / 12 + 1e-15).all()


def cpu_chain():
    """The chain in float64 on the CPU (tests/test_hip_smooth_stream.py's cpu_chain with the limit step between the path and the
    composition): window planes, stability in; the motion in frame pixels, the path and the corrections; the identity field under
    align_corners=True, the reference's levels, sweeps and limited corrections at k = 0.97; the frames warped by the composed field, their
    planes, stability out -- once unlimited, once limited.  Returns the figures of this file's header."""
    import torch.nn.functional as F
    from oracle import frameio_ref

    import limit_ref as L
    import motion_ref as R
    import path_ref as P
    clip = _clip_u8(T, H, W, 21)
    planes = np.stack([frameio_ref.window_plane(f, 256) for f in clip])
    s_in = R.stability_scores(R.global_motion(planes)[0])["stability"]
    motion, _ = P.global_motion_scaled(planes, (W / 256.0, H / 256.0))
    _, D = P.path_smooth(motion, SIGMA)
    u, v = np.meshgrid(np.linspace(-1, 1, 256), np.linspace(-1, 1, 256))
    field = np.stack([np.stack([u, v], -1)] * T)
    rect = L.rectangle(K, (H, W), (256, 256))
    unl = L.reach_bounds(field, D[:, None, :], (H, W), rect, True, 0)
    d_lim, strength, need, left = L.limit_path(D, field, (H, W), K, LEVELS, RELAX, align_corners=True)

    def score(d):
        comp = torch.from_numpy(P.compose64(field, d, (H, W)))
        grid = F.interpolate(comp.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        out = F.grid_sample(torch.from_numpy(clip).permute(0, 3, 1, 2).double(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        out = out.permute(0, 2, 3, 1).clamp(0, 255).floor().to(torch.uint8).numpy()
        planes_out = np.stack([frameio_ref.window_plane(f, 256) for f in out])
        return R.stability_scores(R.global_motion(planes_out)[0])["stability"]
    return {"stability_in": s_in, "stability_out_unlimited": score(D), "stability_out_limited": score(d_lim),
            "reach_px": (float(np.abs(D[:, 2]).max()), float(np.abs(D[:, 5]).max())), "rectangle": rect,
            "unlimited_uncovered_frames": (int((unl[0][:, 0] > 0).sum()), int((unl[1][:, 0] > 0).sum())), "unlimited_uncovered_max": int(unl[1].max()),
            "need": need.tolist(), "frames_needing_limit": int((need < LEVELS).sum()), "strength_min": float(strength.min()),
            "strength_mean": float(strength.mean()), "frames_below_1": int((strength < 1).sum()), "limited_uncovered_max": int(left[1].max())}


def test_a_limited_clip_still_comes_out_steadier(hip, net, clip):
    """The budget costs some smoothness and not the effect: the limited run scores above the geometric mean of the score going in and the
    CPU chain's limited score (0.2730 in, 0.3550 out limited, gate 0.3113), and the clip scores below it going in."""
    from pwstablenet_amd.stream import VideoStabilizer
    vs = VideoStabilizer(net, batch=8, metrics=True, smooth=SIGMA, max_crop=CROP)
    out = vs.run_video(clip, chunk=CHUNK)
    assert out.shape == clip.shape
    rep = vs.stability_report()
    s_in, s_out = rep["stability_in"]["stability"], rep["stability_out"]["stability"]
    print("stability in %.4f (CPU %.4f), out %.4f (CPU limited %.4f), gate %.4f; strength min %.3f"
          % (s_in, CPU_STABILITY_IN, s_out, CPU_STABILITY_OUT_LIMITED, GATE, float(vs.limit_strength.min())))
    assert rep["unfit_pairs_in"] == rep["unfit_pairs_out"] == 0
    assert s_in < GATE < s_out


class _Stub:
    """A generator stand-in for the argument checks, which come before any generator call."""

    def __call__(self, x, is_training):
        raise AssertionError("the generator must not run")


def test_limit_errors(hip):
    from pwstablenet_amd import stream as S
    from pwstablenet_amd.stream import VideoStabilizer
    with pytest.raises(ValueError, match="needs smooth"):
        VideoStabilizer(_Stub(), max_crop=0.05)
    for bad in (-0.01, 0.51, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="max_crop"):
            VideoStabilizer(_Stub(), smooth=SIGMA, max_crop=bad)
    for bad in (0, 65, -3, 2.5, "x", None):
        with pytest.raises(ValueError, match="limit_levels"):
            VideoStabilizer(_Stub(), smooth=SIGMA, max_crop=0.05, limit_levels=bad)
    for bad in (0.0, -0.1, 1.01, float("nan"), "x"):
        with pytest.raises(ValueError, match="limit_relax"):
            VideoStabilizer(_Stub(), smooth=SIGMA, max_crop=0.05, limit_relax=bad)
    ok = VideoStabilizer(_Stub(), smooth=SIGMA, max_crop=0.0, limit_levels=64, limit_relax=1.0)
    assert (ok.max_crop, ok.limit_levels, ok.limit_relax) == (0.0, 64, 1.0) and VideoStabilizer(_Stub(), smooth=SIGMA, max_crop=0.5).max_crop == 0.5
    assert VideoStabilizer(_Stub()).max_crop is None
    # smooth's own refusals are untouched, and the attributes are checked again by the call
    frames = torch.zeros((34, H, W, 3), dtype=torch.uint8, device="cuda")
    vs = VideoStabilizer(_Stub(), batch=8, smooth=SIGMA, max_crop=0.05)
    with pytest.raises(ValueError, match="whole clip"):
        vs.run_video(frames, halo_left=2)
    for borders in ("keep", "mosaic"):
        with pytest.raises(ValueError, match=borders):
            VideoStabilizer(_Stub(), batch=8, smooth=SIGMA, max_crop=0.05, borders=borders).run_video(frames)
    vs.smooth = 0.0
    with pytest.raises(ValueError, match="needs smooth"):
        vs.run_video(frames)
    # the step on its own
    d = torch.zeros((3, 6), dtype=torch.float64, device="cuda")
    f = torch.zeros((3, 8, 8, 2), device="cuda")
    for kw, match in (({"fraction": 0.0}, "fraction"), ({"fraction": 1.5}, "fraction"), ({"levels": 0}, "limit_levels"), ({"relax": 0.0}, "limit_relax"),
                      ({"rolling_shutter": 2.0}, "rolling_shutter"), ({"mode": "nearest"}, "mode"), ({"scene_cuts": [5]}, "scene_cuts")):
        args = dict(fraction=0.9)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            S.limit_path(d, f, (H, W), **args)
    with pytest.raises(ValueError, match="d must"):
        S.limit_path(d[:2], f, (H, W), 0.9)
    with pytest.raises(ValueError, match="fields must"):
        S.limit_path(d, f[:, :1], (H, W), 0.9)
    empty = S.limit_path(d[:0], f[:0], (H, W), 0.9)
    assert [tuple(t.shape) for t in empty] == [(0, 6), (0,), (0,), (0,)]


def main():
    for k, v in cpu_chain().items():
        print(k, v)


if __name__ == "__main__":
    main()
