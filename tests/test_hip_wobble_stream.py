"""GPU tests of wobble suppression in the streaming stabiliser: VideoStabilizer(wobble=sigma).run_video against the frames assembled by hand
from the same steps, in the documented order -- pass 1's fields -> field_homography (the raw fit) -> [functional.rigid_fields] ->
functional.wobble_fields under the call's cuts -> [grid_sample of the planes -> global_motion -> smooth_path -> compose_fields] ->
field_homography again (bounds for crop and zoom) -> [zoom_fields] -> the format's fused warp -> [the crop] -- bit for bit.  The harness of
test_hip_rigid_stream.py: the ngf-16 W1 generator on a smooth synthetic clip, T = 40 at the fit's smallest lattice size 600 x 300, batch 8,
chunks of 16 = two generator batches of 8."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref as R  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402

T, H, W = 40, 300, 600
CHUNK = 16
SIGMA = 2.0


@functools.lru_cache(maxsize=None)
def _net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    net = define_G(31, 2, 16, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=16)})
    return net.cuda()


class _Wobbly:
    """The generator with white noise of a known amplitude added to every field it returns: injected wobble.  The noise comes from a
    generator of its own, so two instances with the same seed, called in the same order, return the same fields."""

    def __init__(self, net, amplitude, seed):
        self.net, self.amplitude = net, amplitude
        self.align_corners = bool(getattr(getattr(net, "module", net), "align_corners", False))
        self.gen = torch.Generator(device="cuda")
        self.gen.manual_seed(seed)

    def __call__(self, x, is_training):
        f = self.net(x, is_training)
        return f + self.amplitude * torch.randn(f.shape, generator=self.gen, device=f.device, dtype=f.dtype)


@functools.lru_cache(maxsize=None)
def _clip(fmt):
    """One smooth scene under small per-frame translations (synth.smooth_frames_u8), as BGR or NV12 frames."""
    base = synth.smooth_frames_u8(1, T, H, W, 17)[0]
    rs = np.random.RandomState(17)
    if fmt == "bgr24":
        col = np.stack([base * 0.9, base * 1.0, base * 0.8], -1) + rs.randint(-3, 4, (T, H, W, 3))
        out = np.clip(col, 0, 255).astype(np.uint8)
    else:
        _, u, v = R.unpack(R.random_yuv(T, H, W, "i420", seed=17), "i420")
        out = R.pack(16 + base.astype(np.int64) * 219 // 255, u, v, fmt)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _dev(fmt):
    return torch.from_numpy(np.array(_clip(fmt))).cuda()


def _planes(src, fmt):
    from pwstablenet_amd import stream as S
    return S.window_planes(src) if fmt == "bgr24" else S.window_planes_yuv(src, fmt)


def _raw_fields(vs, fmt, cuts=None):
    """Pass 1's generator calls: per chunk, on the chunk's planes and what its windows reach, the batches restarting at a cut."""
    planes = _planes(_dev(fmt), fmt)
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    half = vs.period // 2
    with torch.no_grad():
        for cs in range(0, T, CHUNK):
            ce = min(T, cs + CHUNK)
            hl, hr = min(half, cs), min(half, T - ce)
            sc = [t - (cs - hl) for t in (cuts or []) if cs - hl < t < ce + hr] or None
            vs._fields(planes[cs - hl:ce + hr], hl, hr, fields[cs:ce], sc)
    return planes, fields


def _by_hand(vs, fmt, cuts=None, crop=None, zoom=None):
    """(frames, removed, unfit, the fields that warp) from the steps, in the documented order."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    src = _dev(fmt)
    planes, fields = _raw_fields(vs, fmt, cuts)
    m = S.field_homography(fields, (H, W))[0]                      # the raw fit
    if vs.rigidity > 0:
        fields = PF.rigid_fields(fields, m, (H, W), vs.rigidity)
    fields, removed, unfit = PF.wobble_fields(fields, m, (H, W), vs.wobble, scene_cuts=cuts, return_stats=True)
    kw = dict(align_corners=vs.align_corners, mode=vs.interpolation)
    if vs.smooth > 0:                                              # smoothing measures the filtered fields
        seen = PF.grid_sample(planes.unsqueeze(1), fields, align_corners=vs.align_corners).squeeze(1)
        motion, _ = S.global_motion(seen, pixel_scale=(W / 256.0, H / 256.0))
        d, _ = S.smooth_path(motion, vs.smooth, scene_cuts=cuts)
        assert torch.equal(d.view(torch.int64), vs.smooth_correction.view(torch.int64))
        fields = PF.compose_fields(fields, d, (H, W), **kw)
    bounds = S.field_homography(fields, (H, W))[1]                 # the refit: crop and zoom describe the field that warps
    assert bool(torch.isfinite(bounds).all())
    if zoom == "auto":
        window = S.zoom_window(S.auto_crop_window(bounds, (H, W), None, vs.period, scene_cuts=cuts), (H, W))
        assert vs.zoom_windows == [window] * T
        fields = PF.zoom_fields(fields, window, (H, W), **kw)
    out = PF.warp(src, fields, PF.frame_format(fmt, src, "test"), swap_rb=vs.swap_rb, **kw)
    if crop == "auto":
        c = S.auto_crop_window(bounds, (H, W), (H, W), vs.period, scene_cuts=cuts)
        if fmt == "bgr24":
            out = out[:, int(c[2]):int(c[3]), int(c[0]):int(c[1])]
    return out, removed, unfit, fields


def _same(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(torch.uint8) == b.view(torch.uint8)).all())


CASES = [("bgr24", {}, {}), ("bgr24", {"rigidity": 0.5}, {}), ("bgr24", {"smooth": 4.0}, {}), ("bgr24", {}, {"crop": "auto"}),
         ("bgr24", {}, {"zoom": "auto"}), ("bgr24", {}, {"scene_cuts": [20]}), ("bgr24", {}, {"in_flight": 2}),
         ("nv12", {"interpolation": "bicubic"}, {}), ("bgr24", {"smooth": 4.0, "rigidity": 0.5}, {"crop": "auto", "scene_cuts": [13, 29]})]
IDS = ["%s-%s" % (f, "-".join("%s=%s" % kv for kv in list(c.items()) + list(k.items())) or "plain") for f, c, k in CASES]


@pytest.mark.parametrize("fmt,ctor,call", CASES, ids=IDS)
def test_frames_are_the_by_hand_assembly(hip, fmt, ctor, call):
    from pwstablenet_amd.stream import VideoStabilizer
    src = _dev(fmt)
    vs = VideoStabilizer(_net(), batch=8, swap_rb=True, wobble=SIGMA, **ctor)
    got = vs.run_video(src, chunk=CHUNK, pixel_format=fmt, **call)
    want, removed, unfit, _ = _by_hand(vs, fmt, call.get("scene_cuts"), call.get("crop"), call.get("zoom"))
    assert got.is_cuda and _same(got, want)
    assert vs.wobble_removed.is_cuda and vs.wobble_removed.dtype == torch.float32 and tuple(vs.wobble_removed.shape) == (T,)
    assert torch.equal(vs.wobble_removed.view(torch.int32), removed.view(torch.int32))
    assert vs.wobble_unfit.dtype == torch.int32 and torch.equal(vs.wobble_unfit, unfit) and int(unfit.sum()) == 0
    assert float(removed.min()) > 0
    if not ctor and not call:
        plain = VideoStabilizer(_net(), batch=8, swap_rb=True)
        assert not _same(got, plain.run_video(src, chunk=CHUNK))   # the filter changes the frames of this clip
        # from pinned host memory: the same bytes
        host = vs.run_video(src.cpu().pin_memory(), chunk=CHUNK)
        torch.cuda.synchronize()
        assert not host.is_cuda and _same(host, want)


def test_wobble_zero_is_the_default_path(hip):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.stream import VideoStabilizer
    src = _dev("bgr24")
    plain = VideoStabilizer(_net(), batch=8, swap_rb=True)
    zero = VideoStabilizer(_net(), batch=8, swap_rb=True, wobble=0.0)
    assert plain.wobble == zero.wobble == 0.0
    calls, real = [], PF.wobble_fields
    PF.wobble_fields = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        for kw in ({}, {"crop": "auto"}, {"zoom": "auto", "in_flight": 2}):
            assert _same(zero.run_video(src, chunk=CHUNK, **kw), plain.run_video(src, chunk=CHUNK, **kw))
            assert zero.wobble_removed is None and zero.wobble_unfit is None and plain.wobble_removed is None and plain.wobble_unfit is None
        assert not calls   # no launch
        # a call that filtered leaves nothing behind for one that does not
        vs = VideoStabilizer(_net(), batch=8, swap_rb=True, wobble=SIGMA)
        vs.run_video(src, chunk=CHUNK)
        assert calls and vs.wobble_removed is not None and vs.wobble_unfit is not None
        vs.wobble = 0.0
        assert _same(vs.run_video(src, chunk=CHUNK), plain.run_video(src, chunk=CHUNK)) and vs.wobble_removed is None and vs.wobble_unfit is None
    finally:
        PF.wobble_fields = real


class _Stub:
    """A generator stand-in for the argument checks, which come before any generator call."""

    def __call__(self, x, is_training):
        raise AssertionError("the generator must not run")


def test_wobble_errors(hip):
    from pwstablenet_amd.stream import VideoStabilizer
    for bad in (5.5, -0.1, float("nan"), "much"):
        with pytest.raises(ValueError, match="wobble"):
            VideoStabilizer(_Stub(), batch=8, wobble=bad)
    frames = torch.zeros((34, H, W, 3), dtype=torch.uint8, device="cuda")
    vs = VideoStabilizer(_Stub(), batch=8, wobble=SIGMA)
    with pytest.raises(ValueError, match="whole clip"):
        vs.run_video(frames, halo_left=4)
    with pytest.raises(ValueError, match="whole clip"):
        vs.run_video(frames, halo_right=2)
    for borders in ("keep", "mosaic"):
        with pytest.raises(ValueError, match="second pass"):
            VideoStabilizer(_Stub(), batch=8, wobble=SIGMA, borders=borders).run_video(frames)
    with pytest.raises(ValueError, match="600 x 300"):
        vs.run_video(torch.zeros((34, 256, 256, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="600 x 300"):
        vs.run_video(torch.zeros((34, 296 * 3 // 2, 640), dtype=torch.uint8, device="cuda"), pixel_format="nv12")
    vs.wobble = 7.0   # (set after construction)
    with pytest.raises(ValueError, match="wobble"):
        vs.run_video(frames)
    with pytest.raises(TypeError):   # run(), the single-pass entry, does not take it
        vs.run(torch.zeros((34, 256, 256), device="cuda"), frames, wobble=SIGMA)


def _second_difference(e):
    return float((e[2:] - 2 * e[1:-1] + e[:-2]).abs().mean())


def test_injected_wobble_is_removed(hip):
    """White noise of 2e-3 (0.6 pixel at this width) on every field the generator returns: the filter reports what it took out, and the
    residual's mean temporal second difference falls.  Direction only; the ratio is printed.  Measured on an MI355X: removed 2.06 .. 3.51
    pixels per frame, the second difference 4.0e-3 -> 1.2e-4, ratio 0.030."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    from pwstablenet_amd.stream import VideoStabilizer
    src = _dev("bgr24")
    vs = VideoStabilizer(_Wobbly(_net(), 2e-3, 5), batch=8, swap_rb=True, wobble=SIGMA)
    got = vs.run_video(src, chunk=CHUNK)
    assert float(vs.wobble_removed.min()) > 0 and int(vs.wobble_unfit.sum()) == 0
    hand = VideoStabilizer(_Wobbly(_net(), 2e-3, 5), batch=8, swap_rb=True, wobble=SIGMA)   # the same noise, in the same order
    _, raw = _raw_fields(hand, "bgr24")
    m = S.field_homography(raw, (H, W))[0]
    filt, removed, _ = PF.wobble_fields(raw, m, (H, W), SIGMA, return_stats=True)
    assert torch.equal(removed.view(torch.int32), vs.wobble_removed.view(torch.int32))
    assert _same(got, PF.warp(src, filt, PF.frame_format("bgr24", src, "test"), swap_rb=True, align_corners=hand.align_corners, mode="bilinear"))
    P = PF.rigid_fields(raw, m, (H, W), 1.0)   # the homographies' own positions
    before, after = _second_difference(raw - P), _second_difference(filt - P)
    print("injected wobble 2e-3: removed %.3f .. %.3f px per frame; the residual's mean temporal second difference %.3g -> %.3g, ratio %.3f"
          % (float(removed.min()), float(removed.max()), before, after, after / before))
    assert after < before
