"""GPU tests of the 4:2:0 YUV path of the streaming stabiliser (NV12 / I420 in, the same layout out) against the numpy restatement
tests/yuv_ref.py: the gray window planes bit for bit against those of the BGR decode, the fused YUV warp within 1 LSB (BT.601 black
padding), the plane-wise output resize, and run_video / run with pixel_format."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref as R  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402

FMTS = ["nv12", "i420"]


def make_net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    net = define_G(31, 2, 16, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=16)})
    return net.cuda()


def smooth_field(n, seed, scale=1.02, shift=0.01, noise=0.01):
    import torch.nn.functional as F
    rs = np.random.RandomState(seed)
    theta = torch.tensor([[scale, 0.03, shift, -0.02, 2.0 - scale - 0.01, 0.02]]).repeat(n, 1).view(n, 2, 3)
    return (F.affine_grid(theta, (n, 1, 256, 256), align_corners=False)
            + noise * torch.from_numpy(rs.standard_normal((n, 256, 256, 2)).astype(np.float32))).contiguous()


def identity_field(n):
    g = torch.linspace(-1, 1, 256)
    return torch.stack(torch.meshgrid(g, g, indexing="xy"), -1).expand(n, 256, 256, 2).contiguous()


def assert_close_to_ref(got, ref_u8, ref_f, share=6e-2):
    """<= 1 LSB from the float64 restatement, only where its value sits near an integer (fp32 coordinates, as the BGR byte warp's test),
    and at most the BGR test's share of +-1 bytes."""
    diff = np.abs(got.astype(np.int32) - ref_u8.astype(np.int32))
    assert diff.max() <= 1
    assert bool((np.abs(ref_f - np.round(ref_f)) < 0.05)[diff > 0].all())
    assert (diff > 0).mean() < share


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("hw", [(720, 1280), (1080, 1920), (480, 854), (48, 64)])
def test_window_planes_yuv_equal_bgr_decode(hip, fmt, hw):
    from pwstablenet_amd.stream import window_planes, window_planes_yuv
    h, w = hw
    size = min(256, h)   # (INTER_AREA down-scales only: the small frame gets a 48 x 48 plane)
    f = R.random_yuv(2, h, w, fmt, seed=h + w)
    got = window_planes_yuv(torch.from_numpy(f).cuda(), fmt, size)
    via_bgr = window_planes(torch.from_numpy(R.yuv2bgr(f, fmt)).cuda(), size)
    assert torch.equal(got, via_bgr)
    if h <= 480:
        assert np.array_equal(got.cpu().numpy(), R.window_planes(f, fmt, size))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("shape", [(2, 720, 1280), (1, 90, 896), (2, 48, 64), (1, 38, 52)])
def test_yuv_warp_matches_restatement(hip, fmt, ac, shape):
    from pwstablenet_amd import functional as PF
    n, h, w = shape
    f = R.random_yuv(n, h, w, fmt, seed=h)
    field = smooth_field(n, seed=h)
    got = PF.upsample_grid_sample_yuv420(torch.from_numpy(f).cuda(), field.cuda(), fmt, align_corners=ac).cpu().numpy()
    ref, ref_f = R.warp_yuv(f, field.numpy(), fmt, ac, return_float=True)
    assert got.shape == f.shape
    assert_close_to_ref(got, ref, ref_f)


@pytest.mark.parametrize("fmt", FMTS)
def test_yuv_warp_border_reads_black(hip, fmt):
    from pwstablenet_amd import functional as PF
    n, h, w = 2, 72, 128
    f = R.random_yuv(n, h, w, fmt, seed=7)
    field = smooth_field(n, seed=8, scale=1.3, shift=0.4, noise=0.0)   # moves a wide band on the right out of the frame
    got = PF.upsample_grid_sample_yuv420(torch.from_numpy(f).cuda(), field.cuda(), fmt).cpu().numpy()
    ref, ref_f = R.warp_yuv(f, field.numpy(), fmt, False, return_float=True)
    assert_close_to_ref(got, ref, ref_f)
    # where every tap lies outside the plane the restatement's blend is exactly black: the kernel's bytes are black there too
    for g, r, pad in zip(R.unpack(got, fmt), R.unpack(ref_f, fmt), (16, 128, 128)):
        outside = r == pad
        assert outside.mean() > 0.05 and (g[outside] == pad).all()
    y, u, v = R.unpack(got, fmt)
    black = (y == 16) & np.repeat(np.repeat((u == 128) & (v == 128), 2, 1), 2, 2)
    assert black.mean() > 0.05 and (R.yuv2bgr(got, fmt)[black] == 0).all()


@pytest.mark.parametrize("fmt", FMTS)
def test_yuv_warp_identity(hip, fmt):
    """The align_corners=True identity maps every pixel of every plane onto itself.  fp32 coordinates of the resized field land within
    ~1e-4 pixels of the integer, so the truncated blend is the input byte or, where the coordinate falls short and the left neighbour
    is darker, one below it; a field at the luma plane's own power-of-two size (align_corners=False) has exact coordinates: byte for byte."""
    from pwstablenet_amd import functional as PF
    n, h, w = 2, 720, 1280
    f = R.random_yuv(n, h, w, fmt, seed=11)
    got = PF.upsample_grid_sample_yuv420(torch.from_numpy(f).cuda(), identity_field(n).cuda(), fmt, align_corners=True).cpu().numpy()
    d = f.astype(np.int32) - got.astype(np.int32)
    assert d.min() >= 0 and d.max() <= 1
    n, h, w = 2, 128, 256
    f = R.random_yuv(n, h, w, fmt, seed=12, smooth=False)
    xs, ys = (torch.arange(w) * 2 + 1) / w - 1, (torch.arange(h) * 2 + 1) / h - 1
    exact = torch.stack(torch.meshgrid(xs, ys, indexing="xy"), -1).expand(n, h, w, 2).contiguous().float()
    got = PF.upsample_grid_sample_yuv420(torch.from_numpy(f).cuda(), exact.cuda(), fmt, align_corners=False).cpu().numpy()
    assert np.array_equal(R.unpack(got, fmt)[0], R.unpack(f, fmt)[0])
    ref, ref_f = R.warp_yuv(f, exact.numpy(), fmt, False, return_float=True)
    assert_close_to_ref(got, ref, ref_f, share=0.2)   # (uniform noise: no smoothness to keep the near-integer share small)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [(640, 360), (426, 240), (320, 180)])
def test_area_resize_yuv(hip, fmt, size):
    from pwstablenet_amd.stream import area_resize_yuv
    f = R.random_yuv(2, 720, 1280, fmt, seed=size[0])
    got = area_resize_yuv(torch.from_numpy(f).cuda(), fmt, size).cpu().numpy()
    assert np.array_equal(got, R.area_resize_yuv(f, fmt, size))


def shaky_yuv(T, h, w, fmt, seed=3):
    """A shaky clip: one smooth scene under small per-frame translations (synth.smooth_frames_u8) as Y, with smooth chroma."""
    y = synth.smooth_frames_u8(1, T, h, w, seed)[0]
    y = (16 + y.astype(np.int32) * 219 // 255).astype(np.uint8)
    c = R.random_yuv(T, h, w, "i420", seed=seed)
    _, u, v = R.unpack(c, "i420")
    return R.pack(y, u, v, fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_run_video_yuv(hip, fmt):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.distributed import shard_frames
    from pwstablenet_amd.stream import VideoStabilizer, window_planes_yuv
    net = make_net()
    T, h, w = 12, 360, 640
    f = shaky_yuv(T, h, w, fmt)
    d = torch.from_numpy(f).cuda()
    vs = VideoStabilizer(net, batch=16)
    got = vs.run_video(d, chunk=16, pixel_format=fmt)
    assert got.is_cuda and got.shape == d.shape and got.dtype == torch.uint8
    # fields: those of the BGR decode (the window planes are equal bit for bit, test above), in run()'s batches
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    with torch.no_grad():
        vs._fields(window_planes_yuv(d, fmt), 0, 0, fields)
    assert torch.equal(got, PF.upsample_grid_sample_yuv420(d, fields, fmt, align_corners=vs.align_corners))
    ref, ref_f = R.warp_yuv(f, fields.cpu().numpy(), fmt, vs.align_corners, return_float=True)
    assert_close_to_ref(got.cpu().numpy(), ref, ref_f)
    # host-pinned input, two chunks in flight, shards with halos
    host = torch.from_numpy(f).pin_memory()
    got_h = vs.run_video(host, chunk=16, pixel_format=fmt)
    assert not got_h.is_cuda and torch.equal(got_h, got.cpu())
    assert torch.equal(vs.run_video(host, chunk=4, in_flight=2, pixel_format=fmt), vs.run_video(host, chunk=4, in_flight=1, pixel_format=fmt))
    # shards: one window per generator call, so that the shards' batches cannot differ from the whole clip's
    one = VideoStabilizer(net, batch=1)
    whole, parts = one.run_video(d, chunk=5, pixel_format=fmt), []
    for r in range(2):
        s, e, rs, re_ = shard_frames(T, r, 2, halo=15)
        parts.append(one.run_video(d[rs:re_], chunk=5, halo_left=s - rs, halo_right=re_ - e, pixel_format=fmt))
    assert torch.equal(torch.cat(parts, 0), whole)
    # run() with prepared planes
    assert torch.equal(vs.run(window_planes_yuv(d, fmt), d, pixel_format=fmt), got)
    # output resize and crop
    half = vs.run_video(d, chunk=16, half_size_output=True, pixel_format=fmt)
    assert torch.equal(half.cpu(), torch.from_numpy(R.area_resize_yuv(got.cpu().numpy(), fmt, (320, 180))))
    cropped = vs.run_video(host, chunk=16, half_size_output=True, crop=(20, 300, 10, 170), pixel_format=fmt)
    ref_c = R.unpack(half.cpu().numpy(), fmt)
    got_c = R.unpack(cropped.numpy(), fmt)
    assert cropped.shape == (T, 160 * 3 // 2, 280)
    assert np.array_equal(got_c[0], ref_c[0][:, 10:170, 20:300])
    for k in (1, 2):
        assert np.array_equal(got_c[k], ref_c[k][:, 5:85, 10:150])
    with pytest.raises(ValueError):
        vs.run_video(d, chunk=16, half_size_output=True, crop=(21, 300, 10, 170), pixel_format=fmt)
    with pytest.raises(ValueError):
        vs.run_video(d, chunk=16, crop=(20, 300, 10, 171), pixel_format=fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_run_video_yuv_auto_crop_and_output_size(hip, fmt):
    from pwstablenet_amd.stream import VideoStabilizer
    net = make_net()
    T, h, w = 40, 720, 1280
    f = shaky_yuv(T, h, w, fmt, seed=5)
    vs = VideoStabilizer(net, batch=16)
    host = torch.from_numpy(f).pin_memory()
    bgr = torch.from_numpy(R.yuv2bgr(f, fmt)).pin_memory()
    win = {}

    def spy(stab, frames, **kw):   # the window run_video(crop="auto") settles on, read from the bounds it fits
        from pwstablenet_amd import stream as S
        real = S.auto_crop_window
        S.auto_crop_window = lambda *a, **k: win.setdefault(len(win), real(*a, **k))
        try:
            return stab.run_video(frames, chunk=16, half_size_output=True, crop="auto", **kw)
        finally:
            S.auto_crop_window = real
    out_bgr = spy(vs, bgr)
    out_yuv = spy(vs, host, pixel_format=fmt)
    assert win[0] == win[1]   # the same fields: the same bounds and window
    x0, x1, y0, y1 = (int(v) for v in win[0][:4])
    ex = (x0 + (x0 & 1), x1 - (x1 & 1), y0 + (y0 & 1), y1 - (y1 & 1))
    assert out_bgr.shape[1:3] == (y1 - y0, x1 - x0)
    assert out_yuv.shape == (T, (ex[3] - ex[2]) * 3 // 2, ex[1] - ex[0])
    assert torch.equal(out_yuv, vs.run_video(host, chunk=16, half_size_output=True, crop=ex, pixel_format=fmt))
    small = vs.run_video(host, chunk=16, output_size=(640, 360), pixel_format=fmt)
    full = vs.run_video(host, chunk=16, pixel_format=fmt)
    assert small.shape == (T, 540, 640)
    assert np.array_equal(small.numpy(), R.area_resize_yuv(full.numpy(), fmt, (640, 360)))


def test_yuv_errors(hip):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.stream import VideoStabilizer, window_planes_yuv
    vs = VideoStabilizer(make_net(), batch=4)
    field = torch.zeros((1, 256, 256, 2), device="cuda")
    ok = torch.zeros((1, 72, 128), dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros((1, 71, 128), dtype=torch.uint8, device="cuda"),    # packed height not H * 3 // 2 of an even H
                torch.zeros((1, 73, 128), dtype=torch.uint8, device="cuda"),    # (odd H: 48.67)
                torch.zeros((1, 72, 127), dtype=torch.uint8, device="cuda"),    # odd W
                torch.zeros((1, 72, 126), dtype=torch.uint8, device="cuda")):   # W not a multiple of 4
        with pytest.raises(ValueError):
            PF.upsample_grid_sample_yuv420(bad, field, "nv12")
        with pytest.raises(ValueError):
            vs.run_video(bad, pixel_format="i420")
    with pytest.raises(ValueError):
        window_planes_yuv(torch.zeros((1, 74, 128), dtype=torch.uint8, device="cuda"), "nv12")
    with pytest.raises(ValueError):
        vs.run_video(ok, pixel_format="nv12", frames_are_rgb=True)
    with pytest.raises(ValueError):
        vs.run_video(ok, pixel_format="p010")
    with pytest.raises(ValueError):
        vs.run_video(ok, pixel_format="nv12", output_size=(126, 45))
