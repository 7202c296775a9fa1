"""GPU tests of the 10-bit 4:2:0 path of the streaming stabiliser (P010 / I010 in, the same layout out), mirroring tests/test_hip_yuv.py
case for case against the numpy restatement tests/yuv16_ref.py: the gray window planes bit for bit against those of the NV12 / I420 clip of
the reduced samples, the fused 16-bit warp within 1 LSB of 10 bits (BT.601 black padding, 64 / 512), the plane-wise output resize, and
run_video / run with pixel_format."""
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

FMTS = ["p010", "i010"]


def make_net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    net = define_G(31, 2, 16, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=16)})
    return net.cuda()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b):
    """torch.equal of two uint16 tensors (compared as int16 words: the same bits)."""
    return a.dtype == b.dtype == torch.uint16 and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("hw", [(720, 1280), (1080, 1920), (480, 854), (48, 64)])
def test_window_planes_yuv16_equal_reduced_clip(hip, fmt, hw):
    from pwstablenet_amd.stream import window_planes_yuv, window_planes_yuv16
    h, w = hw
    size = min(256, h)   # (INTER_AREA down-scales only: the small frame gets a 48 x 48 plane)
    f = R16.random_yuv16(2, h, w, fmt, seed=h + w)
    if fmt == "p010":   # junk in the low 6 bits of every word is ignored
        f = f | np.random.RandomState(h).randint(0, 64, f.shape).astype(np.uint16)
    else:               # words above 1023 are clamped
        f[:, ::7, ::5] = 60000
    got = window_planes_yuv16(dev(f), fmt, size)
    via8 = window_planes_yuv(dev(R16.reduce(f, fmt)), R16.FMT8[fmt], size)
    assert torch.equal(got, via8)
    if h <= 480:
        assert np.array_equal(got.cpu().numpy(), R16.window_planes(f, fmt, size))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("shape", R16.WARP_SHAPES)
def test_yuv16_warp_matches_restatement(hip, fmt, ac, shape):
    """Against the float64 restatement with yuv16_ref.accept: at most 1 LSB of 10 bits off, only where the float64 blend lies within 0.05
    of an integer, on fewer than 6e-2 of the samples (band and cap of the 8-bit test).  The inputs are yuv16_ref.warp_case's, on which the
    restatement run in float32 passes the same function (tests/test_yuv16_ref_cpu.py)."""
    from pwstablenet_amd import functional as PF
    f, field = R16.warp_case(shape, fmt)
    got = PF.upsample_grid_sample_yuv420_16(dev(f), dev(field), fmt, align_corners=ac)
    assert got.dtype == torch.uint16 and tuple(got.shape) == f.shape
    got = got.cpu().numpy()
    ref, ref_f = R16.warp_yuv(f, field, fmt, ac, return_float=True)
    share = R16.accept(got, ref, ref_f, fmt)
    print("share of samples 1 LSB off %s ac=%s %s: %.2e" % (fmt, ac, shape, share))
    if fmt == "p010":
        assert (got & 63 == 0).all()
    else:
        assert got.max() <= 1023


@pytest.mark.parametrize("fmt", FMTS)
def test_yuv16_warp_border_reads_black(hip, fmt):
    from pwstablenet_amd import functional as PF
    f, field = R16.border_case(fmt)   # moves a wide band on the right out of the frame
    if fmt == "p010":
        f = f | np.random.RandomState(1).randint(0, 64, f.shape).astype(np.uint16)   # input junk must not reach the output
    got = PF.upsample_grid_sample_yuv420_16(dev(f), dev(field), fmt).cpu().numpy()
    ref, ref_f = R16.warp_yuv(f, field, fmt, False, return_float=True)
    R16.accept(got, ref, ref_f, fmt)
    # where every tap lies outside the plane the restatement's blend is exactly black: the kernel's words are black there too, in the
    # format's placement
    shift = 6 if fmt == "p010" else 0
    y, u, v = R.unpack(got, R16.FMT8[fmt])   # (the raw words, plane by plane)
    for g, r, pad in zip((y, u, v), R.unpack(ref_f, R16.FMT8[fmt]), (64, 512, 512)):
        outside = r == pad
        assert outside.mean() > 0.05 and (g[outside] == pad << shift).all()
    if fmt == "p010":
        assert (got & 63 == 0).all()
    black = (y == 64 << shift) & np.repeat(np.repeat((u == 512 << shift) & (v == 512 << shift), 2, 1), 2, 2)
    assert black.mean() > 0.05 and (R.yuv2bgr(R16.reduce(got, fmt), R16.FMT8[fmt])[black] == 0).all()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("ac", [False, True])
def test_yuv16_warp_wide_border(hip, fmt, ac):
    """A 720p clip under a field that zooms out: tap pairs straddle every edge of the 1280-wide Y plane and the 640-wide chroma planes (the
    chroma planes' field access of a wide frame included), which test_yuv16_warp_matches_restatement's wide shapes leave out.
    yuv16_ref.accept_wide: at most 1 LSB of 10 bits off everywhere, the 0.05 band where all four taps are inside, exactly black where all
    are outside; the float32 restatement passes the same (tests/test_yuv16_ref_cpu.py)."""
    from pwstablenet_amd import functional as PF
    f, field = R16.wide_border_case(fmt)
    got = PF.upsample_grid_sample_yuv420_16(dev(f), dev(field), fmt, align_corners=ac).cpu().numpy()
    ref, ref_f = R16.warp_yuv(f, field, fmt, ac, return_float=True)
    inside, outside = R16.tap_masks(f.shape, field, fmt, ac)
    assert outside.mean() > 0.01 and (~inside & ~outside).mean() > 1e-3
    share, straddle = R16.accept_wide(got, ref, ref_f, fmt, inside, outside)
    print("share of samples 1 LSB off %s ac=%s wide border: %.2e (straddling an edge: %.2e)" % (fmt, ac, share, straddle))
    if fmt == "p010":
        assert (got & 63 == 0).all()


@pytest.mark.parametrize("fmt", FMTS)
def test_yuv16_warp_identity(hip, fmt):
    """The align_corners=True identity maps every pixel of every plane onto itself up to ~1e-4 pixels of fp32 coordinate: the truncated
    blend is the input sample or, where the coordinate falls short and the neighbour is darker, one below it.  A field at the luma plane's
    own power-of-two size (align_corners=False) has exact coordinates: Y word for word."""
    from pwstablenet_amd import functional as PF
    n, h, w = 2, 720, 1280
    f = R16.random_yuv16(n, h, w, fmt, seed=11)
    g = torch.linspace(-1, 1, 256)
    ident = torch.stack(torch.meshgrid(g, g, indexing="xy"), -1).expand(n, 256, 256, 2).contiguous()
    got = PF.upsample_grid_sample_yuv420_16(dev(f), ident.cuda(), fmt, align_corners=True).cpu().numpy()
    d = R16.samples(f, fmt) - R16.samples(got, fmt)
    assert d.min() >= 0 and d.max() <= 1
    n, h, w = 2, 128, 256
    f = R16.random_yuv16(n, h, w, fmt, seed=12, smooth=False)   # any 16-bit words
    xs, ys = (torch.arange(w) * 2 + 1) / w - 1, (torch.arange(h) * 2 + 1) / h - 1
    exact = torch.stack(torch.meshgrid(xs, ys, indexing="xy"), -1).expand(n, h, w, 2).contiguous().float()
    got = PF.upsample_grid_sample_yuv420_16(dev(f), exact.cuda(), fmt, align_corners=False).cpu().numpy()
    # word for word up to what the format defines away: P010's low bits come out zero, I010 words above 1023 come out 1023
    assert np.array_equal(got[:, :h], R16.place(R16.samples(f[:, :h], fmt), fmt))
    ref, ref_f = R16.warp_yuv(f, exact.numpy(), fmt, False, return_float=True)
    R16.accept(got, ref, ref_f, fmt, share=0.2)   # (uniform noise: no smoothness to keep the near-integer share small)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [(640, 360), (426, 240), (320, 180)])
def test_area_resize_yuv16(hip, fmt, size):
    from pwstablenet_amd.stream import area_resize_yuv16
    f = R16.random_yuv16(2, 720, 1280, fmt, seed=size[0])
    f[:, :64, :64] = R16.place(1023, fmt)   # a block at the top of the range: nothing may clamp at 8 bits
    got = area_resize_yuv16(dev(f), fmt, size)
    assert got.dtype == torch.uint16
    assert np.array_equal(got.cpu().numpy(), R16.area_resize_yuv16(f, fmt, size))


def shaky_yuv16(T, h, w, fmt, seed=3):
    """A shaky clip: one smooth scene under small per-frame translations (synth.smooth_frames_u8) as Y at 10 bits (with two more bits of
    detail below the 8-bit scene), with smooth chroma."""
    y = synth.smooth_frames_u8(1, T, h, w, seed)[0]
    y = 64 + y.astype(np.int64) * 876 // 255
    _, u, v = R16.unpack(R16.random_yuv16(T, h, w, "i010", seed=seed), "i010")
    return R16.pack(y, u, v, fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_run_video_yuv16(hip, fmt):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.distributed import shard_frames
    from pwstablenet_amd.stream import VideoStabilizer, window_planes_yuv16
    net = make_net()
    T, h, w = 12, 360, 640
    f = shaky_yuv16(T, h, w, fmt)
    d = dev(f)
    vs = VideoStabilizer(net, batch=16)
    got = vs.run_video(d, chunk=16, pixel_format=fmt)
    assert got.is_cuda and got.shape == d.shape and got.dtype == torch.uint16
    # fields: those of the reduced clip (the window planes are equal bit for bit, test above), in run()'s batches
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    with torch.no_grad():
        vs._fields(window_planes_yuv16(d, fmt), 0, 0, fields)
    assert same(got, PF.upsample_grid_sample_yuv420_16(d, fields, fmt, align_corners=vs.align_corners))
    # host-pinned input, two chunks in flight, shards with halos
    host = torch.from_numpy(f).pin_memory()
    got_h = vs.run_video(host, chunk=16, pixel_format=fmt)
    assert not got_h.is_cuda and got_h.dtype == torch.uint16 and same(got_h, got.cpu())
    assert same(vs.run_video(host, chunk=4, in_flight=2, pixel_format=fmt), vs.run_video(host, chunk=4, in_flight=1, pixel_format=fmt))
    # shards: one window per generator call, so that the shards' batches cannot differ from the whole clip's
    one = VideoStabilizer(net, batch=1)
    whole, parts = one.run_video(d, chunk=5, pixel_format=fmt), []
    for r in range(2):
        s, e, rs, re_ = shard_frames(T, r, 2, halo=15)
        parts.append(one.run_video(d[rs:re_], chunk=5, halo_left=s - rs, halo_right=re_ - e, pixel_format=fmt))
    assert same(torch.cat(parts, 0), whole)
    # run() with prepared planes
    assert same(vs.run(window_planes_yuv16(d, fmt), d, pixel_format=fmt), got)
    # output resize and crop
    half = vs.run_video(d, chunk=16, half_size_output=True, pixel_format=fmt)
    assert half.dtype == torch.uint16
    assert np.array_equal(half.cpu().numpy(), R16.area_resize_yuv16(got.cpu().numpy(), fmt, (320, 180)))
    cropped = vs.run_video(host, chunk=16, half_size_output=True, crop=(20, 300, 10, 170), pixel_format=fmt)
    ref_c = R16.unpack(half.cpu().numpy(), fmt)
    got_c = R16.unpack(cropped.numpy(), fmt)
    assert cropped.shape == (T, 160 * 3 // 2, 280) and cropped.dtype == torch.uint16 and not cropped.is_cuda
    assert np.array_equal(got_c[0], ref_c[0][:, 10:170, 20:300])
    for k in (1, 2):
        assert np.array_equal(got_c[k], ref_c[k][:, 5:85, 10:150])
    with pytest.raises(ValueError):
        vs.run_video(d, chunk=16, half_size_output=True, crop=(21, 300, 10, 170), pixel_format=fmt)
    with pytest.raises(ValueError):
        vs.run_video(d, chunk=16, crop=(20, 300, 10, 171), pixel_format=fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_run_video_yuv16_auto_crop_and_output_size(hip, fmt):
    from pwstablenet_amd.stream import VideoStabilizer
    net = make_net()
    T, h, w = 40, 720, 1280
    f = shaky_yuv16(T, h, w, fmt, seed=5)
    vs = VideoStabilizer(net, batch=16)
    host = torch.from_numpy(f).pin_memory()
    host8 = torch.from_numpy(R16.reduce(f, fmt)).pin_memory()   # the NV12 / I420 clip of the reduced samples
    win = {}

    def spy(stab, frames, **kw):   # the window run_video(crop="auto") settles on, read from the bounds it fits
        from pwstablenet_amd import stream as S
        real = S.auto_crop_window
        S.auto_crop_window = lambda *a, **k: win.setdefault(len(win), real(*a, **k))
        try:
            return stab.run_video(frames, chunk=16, half_size_output=True, crop="auto", **kw)
        finally:
            S.auto_crop_window = real
    out8 = spy(vs, host8, pixel_format=R16.FMT8[fmt])
    out16 = spy(vs, host, pixel_format=fmt)
    assert win[0] == win[1]   # the same fields: the same bounds and window
    x0, x1, y0, y1 = (int(v) for v in win[0][:4])
    ex = (x0 + (x0 & 1), x1 - (x1 & 1), y0 + (y0 & 1), y1 - (y1 & 1))
    assert out16.shape == out8.shape == (T, (ex[3] - ex[2]) * 3 // 2, ex[1] - ex[0])
    assert out16.dtype == torch.uint16 and out8.dtype == torch.uint8
    assert same(out16, vs.run_video(host, chunk=16, half_size_output=True, crop=ex, pixel_format=fmt))
    small = vs.run_video(host, chunk=16, output_size=(640, 360), pixel_format=fmt)
    full = vs.run_video(host, chunk=16, pixel_format=fmt)
    assert small.shape == (T, 540, 640)
    assert np.array_equal(small.numpy(), R16.area_resize_yuv16(full.numpy(), fmt, (640, 360)))


def test_yuv16_errors(hip):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.stream import VideoStabilizer, area_resize_yuv16, window_planes_yuv16
    vs = VideoStabilizer(make_net(), batch=4)
    field = torch.zeros((1, 256, 256, 2), device="cuda")
    ok = torch.zeros((1, 72, 128), dtype=torch.uint16, device="cuda")
    ok8 = torch.zeros((1, 72, 128), dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros((1, 71, 128), dtype=torch.uint16, device="cuda"),    # packed height not H * 3 // 2 of an even H
                torch.zeros((1, 73, 128), dtype=torch.uint16, device="cuda"),    # (odd H: 48.67)
                torch.zeros((1, 72, 127), dtype=torch.uint16, device="cuda"),    # odd W
                torch.zeros((1, 72, 126), dtype=torch.uint16, device="cuda")):   # W not a multiple of 4
        with pytest.raises(ValueError):
            PF.upsample_grid_sample_yuv420_16(bad, field, "p010")
        with pytest.raises(ValueError):
            vs.run_video(bad, pixel_format="i010")
    with pytest.raises(ValueError):
        window_planes_yuv16(torch.zeros((1, 74, 128), dtype=torch.uint16, device="cuda"), "p010")
    # a tensor whose dtype does not belong to the pixel format
    for fmt in FMTS:
        with pytest.raises(ValueError):
            vs.run_video(ok8, pixel_format=fmt)
        with pytest.raises(ValueError):
            vs.run(torch.zeros((1, 256, 256), device="cuda"), ok8, pixel_format=fmt)
        with pytest.raises(ValueError):
            PF.upsample_grid_sample_yuv420_16(ok8, field, fmt)
        with pytest.raises(ValueError):
            window_planes_yuv16(ok8, fmt)
        with pytest.raises(ValueError):
            area_resize_yuv16(ok8, fmt, (64, 24))
    for fmt in ("nv12", "i420", "bgr24"):
        with pytest.raises(ValueError):
            vs.run_video(ok, pixel_format=fmt)
    with pytest.raises(ValueError):
        vs.run_video(ok, pixel_format="p016")
    with pytest.raises(ValueError):
        PF.upsample_grid_sample_yuv420_16(ok, field, "nv12")
    with pytest.raises(ValueError):
        vs.run_video(ok, pixel_format="p010", frames_are_rgb=True)
    with pytest.raises(ValueError):
        vs.run_video(ok, pixel_format="p010", output_size=(126, 45))
