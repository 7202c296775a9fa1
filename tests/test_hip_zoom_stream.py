"""GPU tests of zoom to fill in the streaming stabiliser: VideoStabilizer.run(zoom=) and run_video(zoom=a fraction / "auto" / "adaptive")
against the frames assembled by hand from the same steps -- fields -> field_homography -> auto_crop_window -> zoom_window (or zoom_schedule)
-> functional.zoom_fields -> the format's fused warp -> the output resize -- bit for bit.  The ngf-16 W1 generator of test_hip_auto_crop.py on
a smooth synthetic clip, T = 36, 360 x 640; chunks of 16 = two generator batches of 8, so that run_video's generator calls see the windows the
by-hand fields were made from."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv16_ref as R16  # noqa: E402
import yuv_ref as R  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402

T, H, W = 36, 360, 640
CUT = 16   # (a chunk's and a batch's first frame: the clip with the cut runs the generator calls the by-hand fields are made from)


@functools.lru_cache(maxsize=None)
def _net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    net = define_G(31, 2, 16, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=16)})
    return net.cuda()


@functools.lru_cache(maxsize=None)
def _clip(fmt):
    """One smooth scene under small per-frame translations (synth.smooth_frames_u8), as BGR, NV12 or P010 frames."""
    base = synth.smooth_frames_u8(1, T, H, W, 17)[0]
    rs = np.random.RandomState(17)
    if fmt == "bgr24":
        col = np.stack([base * 0.9, base * 1.0, base * 0.8], -1) + rs.randint(-3, 4, (T, H, W, 3))
        out = np.clip(col, 0, 255).astype(np.uint8)
    elif fmt == "nv12":
        _, u, v = R.unpack(R.random_yuv(T, H, W, "i420", seed=17), "i420")
        out = R.pack(16 + base.astype(np.int64) * 219 // 255, u, v, fmt)
    else:
        _, u, v = R16.unpack(R16.random_yuv16(T, H, W, "i010", seed=17), "i010")
        out = R16.pack(64 + base.astype(np.int64) * 876 // 255, u, v, fmt)
    out.setflags(write=False)
    return out


def _stab(interpolation="bilinear", net=None):
    from pwstablenet_amd.stream import VideoStabilizer
    return VideoStabilizer(net or _net(), batch=8, swap_rb=True, interpolation=interpolation)


def _planes(src, fmt):
    from pwstablenet_amd import stream as S
    if fmt == "bgr24":
        return S.window_planes(src)
    return S.window_planes_yuv(src, fmt) if fmt == "nv12" else S.window_planes_yuv16(src, fmt)


@functools.lru_cache(maxsize=None)
def _fields(fmt, cuts=()):
    """(fields (T, 256, 256, 2), bounds (T, 4)) of the format's clip, in run()'s batches: computed once, read-only from then on."""
    from pwstablenet_amd.stream import field_homography
    vs = _stab()
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    with torch.no_grad():
        vs._fields(_planes(torch.from_numpy(np.array(_clip(fmt))).cuda(), fmt), 0, 0, fields, list(cuts) or None)
    _, bounds = field_homography(fields, (H, W))
    assert torch.isfinite(bounds).all()
    return fields, bounds


def _by_hand(vs, src, fmt, fields, windows, output_size, return_uncovered=False):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    zf, unc = PF.zoom_fields(fields, windows, (H, W), align_corners=vs.align_corners, mode=vs.interpolation, return_uncovered=True)
    kw = dict(align_corners=vs.align_corners, mode=vs.interpolation)
    if fmt == "bgr24":
        out = PF.upsample_grid_sample_u8(src, zf, swap_rb=vs.swap_rb, **kw)
        out = S.area_resize(out, output_size) if output_size else out
    elif fmt == "nv12":
        out = PF.upsample_grid_sample_yuv420(src, zf, fmt, **kw)
        out = S.area_resize_yuv(out, fmt, output_size) if output_size else out
    else:
        out = PF.upsample_grid_sample_yuv420_16(src, zf, fmt, **kw)
        out = S.area_resize_yuv16(out, fmt, output_size) if output_size else out
    return (out, unc) if return_uncovered else out


def _same(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(torch.uint8) == b.view(torch.uint8)).all())


def _auto_window(bounds, period):
    from pwstablenet_amd.stream import auto_crop_window, zoom_window
    crop = auto_crop_window(bounds, (H, W), None, period)
    window = zoom_window(crop, (H, W))
    x0, x1, y0, y1 = window
    assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H and (x1 - x0 < W or y1 - y0 < H), window   # a real zoom on this clip
    return window


@pytest.mark.parametrize("fmt,interpolation,in_flight,on_host,output_size", [
    ("bgr24", "bilinear", 1, True, None), ("bgr24", "bicubic", 2, False, (320, 180)),
    ("nv12", "bilinear", 2, True, (320, 180)), ("nv12", "bilinear", 1, False, None),
    ("p010", "bilinear", 1, False, (320, 180)), ("p010", "bilinear", 2, True, None)])
def test_run_video_zoom_auto_equals_the_by_hand_assembly(hip, fmt, interpolation, in_flight, on_host, output_size):
    vs = _stab(interpolation)
    fields, bounds = _fields(fmt)
    window = _auto_window(bounds, vs.period)
    dev = torch.from_numpy(np.array(_clip(fmt))).cuda()
    src = torch.from_numpy(np.array(_clip(fmt))).pin_memory() if on_host else dev
    want, unc = _by_hand(vs, dev, fmt, fields, window, output_size, return_uncovered=True)
    got = vs.run_video(src, chunk=16, zoom="auto", in_flight=in_flight, pixel_format=fmt, output_size=output_size)
    torch.cuda.synchronize()
    ow, oh = output_size or (W, H)
    assert tuple(got.shape) == ((T, oh, ow, 3) if fmt == "bgr24" else (T, oh * 3 // 2, ow))   # the size that was asked for
    assert got.is_cuda != on_host and got.dtype == src.dtype
    assert _same(got, want)
    assert vs.zoom_windows == [window] * T
    assert vs.zoom_uncovered.dtype == torch.int32 and vs.zoom_uncovered.is_cuda and torch.equal(vs.zoom_uncovered, unc)
    # the window is fractional: the zoom does not share the crop's even-edge rule
    assert fmt == "bgr24" or any(abs(v - round(v)) > 1e-6 or int(round(v)) & 1 for v in window)


def test_run_video_zoom_adaptive_uses_the_schedule(hip):
    from pwstablenet_amd.stream import zoom_schedule
    fmt = "bgr24"
    vs = _stab()
    fields, bounds = _fields(fmt, (CUT,))
    windows = zoom_schedule(bounds, (H, W), 0.01, 0.6, scene_cuts=[CUT])
    print("adaptive: %d distinct windows, k from %.3f to %.3f" % (len(set(windows)), min(w[1] - w[0] for w in windows) / W, max(w[1] - w[0] for w in windows) / W))
    assert len(set(windows)) > 1
    dev = torch.from_numpy(np.array(_clip(fmt))).cuda()
    got = vs.run_video(dev, chunk=16, zoom="adaptive", zoom_speed=0.01, zoom_min=0.6, scene_cuts=[CUT])
    assert vs.zoom_windows == windows and vs.scene_cuts == [CUT]
    assert tuple(got.shape) == (T, H, W, 3)
    assert _same(got, _by_hand(vs, dev, fmt, fields, windows, None))
    assert _same(got, vs.run_video(dev.cpu().pin_memory(), chunk=16, zoom="adaptive", zoom_speed=0.01, zoom_min=0.6, scene_cuts=[CUT], in_flight=2))


class _Counting:
    """The generator, counting the windows it is called on."""

    def __init__(self, net):
        self.net, self.module, self.windows = net, net.module, 0

    def __call__(self, x, is_training):
        self.windows += x.shape[0]
        return self.net(x, is_training)


@pytest.mark.parametrize("fmt", ["bgr24", "nv12"])
def test_run_video_zoom_fraction_is_one_pass_through_run(hip, fmt):
    from pwstablenet_amd import stream as S
    net = _Counting(_net())
    vs = _stab(net=net)
    dev = torch.from_numpy(np.array(_clip(fmt))).cuda()
    fits, real = [], S._field_homography
    S._field_homography = lambda *a, **k: fits.append(1) or real(*a, **k)
    try:
        got = vs.run_video(dev, chunk=16, zoom=0.9, pixel_format=fmt)
    finally:
        S._field_homography = real
    assert net.windows == T and not fits            # the generator once per frame, no bounds: the single pass
    window = (0.05 * W, 0.95 * W, 0.05 * H, 0.95 * H)
    assert np.allclose(vs.zoom_windows, [window] * T, rtol=0, atol=1e-9)
    unc = vs.zoom_uncovered.clone()
    want = vs.run(_planes(dev, fmt), dev, pixel_format=fmt, zoom=vs.zoom_windows[0])
    assert _same(got, want) and torch.equal(unc, vs.zoom_uncovered) and tuple(unc.shape) == (T,)
    assert _same(got, _by_hand(vs, dev, fmt, _fields(fmt)[0], vs.zoom_windows, None))
    assert _same(got, vs.run_video(dev.cpu().pin_memory(), chunk=16, zoom=0.9, pixel_format=fmt, in_flight=2))
    # per-frame windows through run()
    windows = [(t, W - 2.5 * t, 0.5 * t, H - t) for t in range(T)]
    assert _same(vs.run(_planes(dev, fmt), dev, pixel_format=fmt, zoom=windows), _by_hand(vs, dev, fmt, _fields(fmt)[0], windows, None))
    assert vs.zoom_windows == [tuple(float(v) for v in w) for w in windows]


@pytest.mark.parametrize("fmt", ["bgr24", "p010"])
def test_zoom_one_is_no_zoom_and_auto_uncovers_no_more(hip, fmt):
    vs = _stab()
    dev = torch.from_numpy(np.array(_clip(fmt))).cuda()
    plain = vs.run_video(dev, chunk=16, pixel_format=fmt)
    assert vs.zoom_windows is None and vs.zoom_uncovered is None
    one = vs.run_video(dev, chunk=16, pixel_format=fmt, zoom=1.0)
    assert _same(one, plain)
    assert vs.zoom_windows == [(0.0, float(W), 0.0, float(H))] * T
    unzoomed = int(vs.zoom_uncovered.sum())
    vs.run_video(dev, chunk=16, pixel_format=fmt, zoom="auto")
    zoomed = int(vs.zoom_uncovered.sum())
    print("%s: uncovered field nodes without zoom %d, with zoom=\"auto\" %d" % (fmt, unzoomed, zoomed))
    assert zoomed <= unzoomed


class _Stub:
    """A generator stand-in for the argument checks, which come before any generator call."""

    def __call__(self, x, is_training):
        raise AssertionError("the generator must not run")


def test_zoom_errors(hip):
    from pwstablenet_amd.stream import VideoStabilizer
    frames = torch.zeros((34, H, W, 3), dtype=torch.uint8, device="cuda")
    vs = VideoStabilizer(_Stub(), batch=8)
    for zoom in ("auto", "adaptive", 0.9):
        with pytest.raises(ValueError, match="crop"):
            vs.run_video(frames, zoom=zoom, crop=(0, 640, 0, 360))
        with pytest.raises(ValueError, match="crop"):
            vs.run_video(frames, zoom=zoom, crop="auto")
    for zoom in ("auto", "adaptive"):
        with pytest.raises(ValueError, match="whole clip"):
            vs.run_video(frames, zoom=zoom, halo_left=2)
        with pytest.raises(ValueError, match="whole clip"):
            vs.run_video(frames, zoom=zoom, halo_right=1)
        with pytest.raises(ValueError, match="600 x 300"):
            vs.run_video(frames[:, :296, :600].contiguous(), zoom=zoom)
    for zoom in ("automatic", "", 0.0, -0.1, 1.5, float("nan"), (0, 640, 0, 360)):
        with pytest.raises(ValueError, match="zoom"):
            vs.run_video(frames, zoom=zoom)
    keep = VideoStabilizer(_Stub(), batch=8, borders="keep")
    for zoom in ("auto", "adaptive", 0.9):
        with pytest.raises(ValueError, match="keep"):
            keep.run_video(frames, zoom=zoom)
    with pytest.raises(ValueError, match="keep"):
        keep.run(torch.zeros((34, 256, 256), device="cuda"), frames, zoom=(0, 640, 0, 360))
    with pytest.raises(ValueError):
        vs.run(torch.zeros((34, 256, 256), device="cuda"), frames, zoom=(0, 641, 0, 360))
    with pytest.raises(ValueError):
        vs.run(torch.zeros((34, 256, 256), device="cuda"), frames, zoom=[(0, 640, 0, 360)] * 33)
