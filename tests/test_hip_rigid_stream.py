"""GPU tests of rigid warp mode in the streaming stabiliser: VideoStabilizer(rigidity=r).run / run_video against the frames assembled by hand
from the same steps -- fields -> field_homography -> functional.rigid_fields -> [zoom_fields] -> the format's fused warp -> [keep_borders_]
-> [the output resize / the crop] -- bit for bit.  The harness of test_hip_zoom_stream.py: the ngf-16 W1 generator on a smooth synthetic clip,
T = 36, 360 x 640, batch 8, chunks of 16 = two generator batches of 8, so that run_video's generator calls see the windows the by-hand fields
were made from."""
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

T, H, W = 36, 360, 640


@functools.lru_cache(maxsize=None)
def _net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    net = define_G(31, 2, 16, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=16)})
    return net.cuda()


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


def _dev(fmt):
    return torch.from_numpy(np.array(_clip(fmt))).cuda()


def _stab(rigidity=None, interpolation="bilinear", borders="black", net=None):
    from pwstablenet_amd.stream import VideoStabilizer
    kw = {} if rigidity is None else {"rigidity": rigidity}
    return VideoStabilizer(net or _net(), batch=8, swap_rb=True, interpolation=interpolation, borders=borders, **kw)


def _planes(src, fmt):
    from pwstablenet_amd import stream as S
    return S.window_planes(src) if fmt == "bgr24" else S.window_planes_yuv(src, fmt)


@functools.lru_cache(maxsize=None)
def _fields(fmt):
    """(raw fields (T, 256, 256, 2), M (T, 3, 3), bounds (T, 4)) of the format's clip, in run()'s batches: computed once, read-only."""
    from pwstablenet_amd.stream import field_homography
    vs = _stab()
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    with torch.no_grad():
        vs._fields(_planes(_dev(fmt), fmt), 0, 0, fields)
    m, bounds = field_homography(fields, (H, W))
    assert torch.isfinite(bounds).all()
    return fields, m, bounds


@functools.lru_cache(maxsize=None)
def _rigid(fmt, r):
    """(adjusted fields, residual, unfit) by hand."""
    from pwstablenet_amd import functional as PF
    fields, m, _ = _fields(fmt)
    out, res, unfit = PF.rigid_fields(fields, m, (H, W), r, return_stats=True)
    assert out.data_ptr() != fields.data_ptr() and float(res.min()) > 0 and int(unfit.sum()) == 0
    return out, res, unfit


def _warp(vs, src, fmt, fields, output_size=None):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    kw = dict(align_corners=vs.align_corners, mode=vs.interpolation)
    if fmt == "bgr24":
        out = PF.upsample_grid_sample_u8(src, fields, swap_rb=vs.swap_rb, **kw)
        return S.area_resize(out, output_size) if output_size else out
    out = PF.upsample_grid_sample_yuv420(src, fields, fmt, **kw)
    return S.area_resize_yuv(out, fmt, output_size) if output_size else out


def _same(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(torch.uint8) == b.view(torch.uint8)).all())


def _stats_are(vs, fmt, r):
    _, res, unfit = _rigid(fmt, r)
    return (vs.rigid_residual.dtype == torch.float32 and vs.rigid_residual.is_cuda and tuple(vs.rigid_residual.shape) == (T,)
            and torch.equal(vs.rigid_residual.view(torch.int32), res.view(torch.int32))
            and vs.rigid_unfit.dtype == torch.int32 and vs.rigid_unfit.is_cuda and torch.equal(vs.rigid_unfit, unfit))


def test_run_and_run_video_equal_the_by_hand_assembly(hip):
    fmt = "bgr24"
    dev = _dev(fmt)
    vs = _stab(1.0)
    want = _warp(vs, dev, fmt, _rigid(fmt, 1.0)[0])
    assert not _same(want, _warp(vs, dev, fmt, _fields(fmt)[0]))   # rigidity changes the frames of this clip
    assert _same(vs.run(_planes(dev, fmt), dev), want) and _stats_are(vs, fmt, 1.0)
    print("residual per frame, source pixels: %.3f .. %.3f" % (float(vs.rigid_residual.min()), float(vs.rigid_residual.max())))
    vs = _stab(0.5)
    want = _warp(vs, dev, fmt, _rigid(fmt, 0.5)[0])
    got = vs.run_video(dev, chunk=16)
    assert got.is_cuda and _same(got, want) and _stats_are(vs, fmt, 0.5)
    # in_flight = 2, from pinned host memory: the same bytes and statistics
    got = vs.run_video(dev.cpu().pin_memory(), chunk=16, in_flight=2)
    torch.cuda.synchronize()
    assert not got.is_cuda and _same(got, want) and _stats_are(vs, fmt, 0.5)
    # a shard with halos: nothing in the adjustment depends on other frames
    got = vs.run_video(dev[2:30], chunk=16, halo_left=6, halo_right=4)
    assert tuple(vs.rigid_residual.shape) == (18,) and tuple(got.shape) == (18, H, W, 3)


def test_single_pass_zoom_comes_after_the_adjustment(hip):
    from pwstablenet_amd import functional as PF
    fmt = "bgr24"
    dev = _dev(fmt)
    vs = _stab(0.5)
    got = vs.run_video(dev, chunk=16, zoom=0.9)
    zf, unc = PF.zoom_fields(_rigid(fmt, 0.5)[0], vs.zoom_windows, (H, W), align_corners=vs.align_corners, mode=vs.interpolation, return_uncovered=True)
    assert _same(got, _warp(vs, dev, fmt, zf)) and torch.equal(vs.zoom_uncovered, unc) and _stats_are(vs, fmt, 0.5)


@pytest.mark.parametrize("in_flight,on_host", [(1, False), (2, True)])
def test_run_video_nv12(hip, in_flight, on_host):
    fmt = "nv12"
    dev = _dev(fmt)
    vs = _stab(1.0)
    src = dev.cpu().pin_memory() if on_host else dev
    got = vs.run_video(src, chunk=16, pixel_format=fmt, output_size=(320, 180), in_flight=in_flight)
    torch.cuda.synchronize()
    assert got.is_cuda != on_host and _same(got, _warp(vs, dev, fmt, _rigid(fmt, 1.0)[0], (320, 180))) and _stats_are(vs, fmt, 1.0)


def test_run_video_bicubic(hip):
    fmt = "bgr24"
    dev = _dev(fmt)
    vs = _stab(0.5, interpolation="bicubic")
    got = vs.run_video(dev, chunk=16, output_size=(320, 180))
    assert _same(got, _warp(vs, dev, fmt, _rigid(fmt, 0.5)[0], (320, 180))) and _stats_are(vs, fmt, 0.5)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_run_video_crop_auto_keeps_the_raw_fit_s_bounds(hip, in_flight):
    from pwstablenet_amd.stream import auto_crop_window
    fmt = "bgr24"
    dev = _dev(fmt)
    vs = _stab(1.0)
    x0, x1, y0, y1 = auto_crop_window(_fields(fmt)[2], (H, W), (H, W), vs.period)   # the RAW field's bounds
    assert (int(x1) - int(x0), int(y1) - int(y0)) != (W, H)
    want = _warp(vs, dev, fmt, _rigid(fmt, 1.0)[0])[:, int(y0):int(y1), int(x0):int(x1)]
    got = vs.run_video(dev, chunk=16, crop="auto", in_flight=in_flight)
    assert _same(got, want) and _stats_are(vs, fmt, 1.0)


def test_run_video_zoom_auto(hip):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.stream import auto_crop_window, zoom_window
    fmt = "bgr24"
    dev = _dev(fmt)
    vs = _stab(1.0)
    window = zoom_window(auto_crop_window(_fields(fmt)[2], (H, W), None, vs.period), (H, W))
    zf, unc = PF.zoom_fields(_rigid(fmt, 1.0)[0], window, (H, W), align_corners=vs.align_corners, mode=vs.interpolation, return_uncovered=True)
    got = vs.run_video(dev, chunk=16, zoom="auto")
    assert vs.zoom_windows == [window] * T and torch.equal(vs.zoom_uncovered, unc)
    assert _same(got, _warp(vs, dev, fmt, zf)) and _stats_are(vs, fmt, 1.0)


@pytest.mark.parametrize("fmt", ["bgr24", "nv12"])
def test_borders_keep_sees_the_adjusted_field(hip, fmt):
    from pwstablenet_amd import functional as PF
    dev = _dev(fmt)
    vs = _stab(1.0, borders="keep")
    fields = _rigid(fmt, 1.0)[0]
    want = _warp(vs, dev, fmt, fields).clone()
    PF.keep_borders_(want, fields, dev[0], fmt, initial_is_source=True, swap_rb=vs.swap_rb and fmt == "bgr24", align_corners=vs.align_corners,
                     mode=vs.interpolation)
    assert _same(vs.run_video(dev, chunk=16, pixel_format=fmt), want) and _stats_are(vs, fmt, 1.0)
    assert _same(vs.run_video(dev, chunk=16, pixel_format=fmt, in_flight=2), want)
    assert _same(vs.run(_planes(dev, fmt), dev, pixel_format=fmt), want)


def test_rigidity_zero_is_the_default_path(hip):
    from pwstablenet_amd import stream as S
    from pwstablenet_amd.stream import VideoStabilizer
    fmt = "bgr24"
    dev = _dev(fmt)
    plain = VideoStabilizer(_net(), batch=8, swap_rb=True)
    zero = VideoStabilizer(_net(), batch=8, swap_rb=True, rigidity=0.0)
    assert plain.rigidity == 0.0
    fits, real = [], S._field_homography
    S._field_homography = lambda *a, **k: fits.append(1) or real(*a, **k)
    try:
        got = zero.run_video(dev, chunk=16)
    finally:
        S._field_homography = real
    assert not fits and zero.rigid_residual is None and zero.rigid_unfit is None   # no fit, no launch
    assert _same(got, plain.run_video(dev, chunk=16)) and plain.rigid_residual is None and plain.rigid_unfit is None
    assert _same(got, _warp(zero, dev, fmt, _fields(fmt)[0]))
    assert _same(zero.run(_planes(dev, fmt), dev), got) and zero.rigid_residual is None
    zero.run_video(dev, chunk=16, crop="auto")
    assert zero.rigid_residual is None and zero.rigid_unfit is None


class _Stub:
    """A generator stand-in for the argument checks, which come before any generator call."""

    def __call__(self, x, is_training):
        raise AssertionError("the generator must not run")


def test_rigidity_errors(hip):
    from pwstablenet_amd.stream import VideoStabilizer
    for bad in (1.2, -0.1, float("nan"), "full"):
        with pytest.raises(ValueError, match="rigidity"):
            VideoStabilizer(_Stub(), batch=8, rigidity=bad)
    vs = VideoStabilizer(_Stub(), batch=8, rigidity=0.5)
    small = torch.zeros((34, 256, 256, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="600 x 300"):
        vs.run_video(small)
    with pytest.raises(ValueError, match="600 x 300"):
        vs.run(torch.zeros((34, 256, 256), device="cuda"), small)
    with pytest.raises(ValueError, match="600 x 300"):
        vs.run_video(torch.zeros((34, 296 * 3 // 2, 640), dtype=torch.uint8, device="cuda"), pixel_format="nv12")
