"""GPU test of the stabiliser's per-format selection (functional.FRAME_FORMATS): for every pixel format plus float frames, in both
interpolation modes, VideoStabilizer runs the kernels that the direct functional calls run -- bit for bit (torch.equal), on the very fields
run() forms (VideoStabilizer._fields of the same window planes).  The direct calls are tested against float64 elsewhere; this file asserts
that nothing between ``pixel_format`` and the launch picks another entry, another layout or another plane size.

run() and borders="keep": T = 4 frames of 38 x 52 with the ngf = 16 generator of test_hip_bicubic.make_net.  Chroma is 19 x 26 -- odd chroma
height, chroma width 2 mod 4, and the last sample's exact-load path: the smallest frames at which the table can select wrongly or a merged
launcher can mis-size a plane.  The window planes are synth's (run() takes them as an argument).

run_video (output resize and crop): run_video computes the 256 x 256 window planes itself, and INTER_AREA only scales down, so it takes no
frame below 256 x 256 (tests/test_hip_keep_stream.py says the same).  Those two assertions therefore use 258 x 260 frames -- chroma 129 x 130,
again odd and 2 mod 4, the smallest such size it accepts -- with output_size (130, 128) (half the width; the even height below half, as
(26, 18) is to 52 x 38) and the crop window (2, 24, 2, 16) as it stands.

The stabilisers are built with swap_rb=True: "bgr24" must pass it on, the packed formats must ignore it.  The integer frames are uniform
noise (for 16 bits over all words: junk in P010's low bits, I010 words above 1023), which an equality between two paths can take.
No crop="auto" and no zoom: their 600 x 300 minimum would make this slow, and tests/test_hip_zoom_stream.py / test_hip_auto_crop.py cover them."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hip_bicubic import make_net  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402

T = 4
INTEGER = ("bgr24", "nv12", "i420", "p010", "i010")
MODES = ("bilinear", "bicubic")


@pytest.fixture(scope="module")
def net(hip):
    return make_net()


@pytest.fixture(scope="module")
def small(net):
    """The 38 x 52 case's window planes and the fields run() forms from them (computed once, read only)."""
    from pwstablenet_amd.stream import VideoStabilizer
    gray = torch.from_numpy(synth.make_window(1, T, 256, seed=7)[0]).cuda()
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    with torch.no_grad():
        VideoStabilizer(net, batch=16)._fields(gray, 0, 0, fields)
    return gray, fields


def make_frames(fmt, h, w):
    rs = np.random.RandomState(11)
    if fmt == "float":
        return torch.from_numpy(synth.smooth_frames_u8(T, 3, h, w, 5).astype(np.float32)).cuda()
    if fmt == "bgr24":
        return torch.from_numpy(rs.randint(0, 256, (T, h, w, 3)).astype(np.uint8)).cuda()
    if fmt in ("nv12", "i420"):
        return torch.from_numpy(rs.randint(0, 256, (T, h * 3 // 2, w)).astype(np.uint8)).cuda()
    return torch.from_numpy(rs.randint(0, 65536, (T, h * 3 // 2, w)).astype(np.uint16)).cuda()


def direct_warp(frames, fields, fmt, vs, mode):
    """The functional call a caller without the stabiliser would make for these frames."""
    from pwstablenet_amd import functional as PF
    if fmt == "float":
        return PF.upsample_grid_sample(frames, fields, align_corners=vs.align_corners, mode=mode)
    if fmt == "bgr24":
        return PF.upsample_grid_sample_u8(frames, fields, swap_rb=vs.swap_rb, align_corners=vs.align_corners, mode=mode)
    if fmt in ("nv12", "i420"):
        return PF.upsample_grid_sample_yuv420(frames, fields, fmt, align_corners=vs.align_corners, mode=mode)
    return PF.upsample_grid_sample_yuv420_16(frames, fields, fmt, align_corners=vs.align_corners, mode=mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", INTEGER + ("float",))
def test_run_selects_the_direct_warp(net, small, fmt, mode):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.stream import VideoStabilizer
    gray, fields = small
    frames = make_frames(fmt, 38, 52)
    name = "bgr24" if fmt == "float" else fmt
    vs = VideoStabilizer(net, batch=16, swap_rb=True, interpolation=mode)
    want = direct_warp(frames, fields, fmt, vs, mode)
    got = vs.run(gray, frames, pixel_format=name)
    assert got.shape == frames.shape and got.dtype == frames.dtype and got.is_cuda
    assert torch.equal(got, want)
    assert not torch.equal(got, frames)   # (the field moves the picture: the equality above compares warps, not copies)
    if fmt == "float":
        return
    keep = VideoStabilizer(net, batch=16, swap_rb=True, interpolation=mode, borders="keep").run(gray, frames, pixel_format=name)
    kept = PF.keep_borders_(want.clone(), fields, frames[0], name, initial_is_source=True, swap_rb=vs.swap_rb, align_corners=vs.align_corners,
                            mode=mode)
    assert torch.equal(keep, kept)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", INTEGER)
def test_run_video_resize_and_crop(net, fmt, mode):
    from pwstablenet_amd import stream as S
    h, w, size, crop = 258, 260, (130, 128), (2, 24, 2, 16)
    frames = make_frames(fmt, h, w)
    planes = {"bgr24": lambda f: S.window_planes(f), "nv12": lambda f: S.window_planes_yuv(f, fmt), "i420": lambda f: S.window_planes_yuv(f, fmt),
              "p010": lambda f: S.window_planes_yuv16(f, fmt), "i010": lambda f: S.window_planes_yuv16(f, fmt)}[fmt]
    resize = {"bgr24": lambda f: S.area_resize(f, size), "nv12": lambda f: S.area_resize_yuv(f, fmt, size),
              "i420": lambda f: S.area_resize_yuv(f, fmt, size), "p010": lambda f: S.area_resize_yuv16(f, fmt, size),
              "i010": lambda f: S.area_resize_yuv16(f, fmt, size)}[fmt]
    vs = S.VideoStabilizer(net, batch=16, swap_rb=True, interpolation=mode)
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    gray = planes(frames)
    with torch.no_grad():
        vs._fields(gray, 0, 0, fields)
    full = direct_warp(frames, fields, fmt, vs, mode)
    assert torch.equal(vs.run_video(frames, chunk=16, pixel_format=fmt), full)
    assert torch.equal(vs.run_video(frames, chunk=16, pixel_format=fmt, output_size=size), resize(full))
    x0, x1, y0, y1 = crop
    cropped = vs.run_video(frames, chunk=16, pixel_format=fmt, crop=crop)
    if fmt == "bgr24":
        assert torch.equal(cropped, full[:, y0:y1, x0:x1, :])
        return
    # the window of every plane, packed again: Y rows, then NV12 / P010's interleaved UV rows or I420 / I010's U plane and V plane
    luma, chroma = full[:, :h], full[:, h:].reshape(T, -1)
    if fmt in ("nv12", "p010"):
        parts = [chroma.reshape(T, h // 2, w)[:, y0 // 2:y1 // 2, x0:x1]]
    else:
        parts = [c[:, y0 // 2:y1 // 2, x0 // 2:x1 // 2] for c in chroma.reshape(T, 2, h // 2, w // 2).unbind(1)]
    want = torch.cat([luma[:, y0:y1, x0:x1].reshape(T, -1)] + [c.reshape(T, -1) for c in parts], 1).reshape(T, (y1 - y0) * 3 // 2, x1 - x0)
    assert torch.equal(cropped, want)
