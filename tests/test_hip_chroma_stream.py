"""GPU test of the stabiliser on 4:2:2 and 4:4:4 frames (functional.CHROMA_FORMATS): tests/test_hip_format_matrix.py's two tests for the six
formats -- VideoStabilizer runs the kernels that the direct functional calls run, bit for bit (torch.equal), on the very fields run() forms
-- plus in_flight, zoom and crop="auto" at one or two formats each.  The direct calls are held to the 4:2:0 kernels' bits in
tests/test_hip_chroma_warp.py and test_hip_chroma_planes.py; this file asserts that nothing between ``pixel_format`` and the launches picks
another entry, another layout, another subsampling or another plane size.

run() and borders="keep": T = 4 frames of 38 x 52 (4:2:2 chroma 38 x 26: width 2 mod 4; the last sample's exact loads).  run_video (full,
output_size, crop) at 258 x 260, the smallest frames it takes, with output_size (130, 128) and a crop window with an odd y edge for 4:2:2
and odd x and y edges for 4:4:4 -- what those formats allow and 4:2:0 does not; an odd x edge for 4:2:2 is a ValueError.  Frames are uniform
noise over all words.  crop="auto" runs on 304 x 600 frames (the fit's lattice needs 600 x 300) with test_hip_auto_crop.py's affine
stand-in for the generator, whose bounds are known."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chroma_ref as C  # noqa: E402
from test_hip_auto_crop import _AffineStub  # noqa: E402
from test_hip_bicubic import make_net  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402

T = 4
NAMES = tuple(C.FORMATS)
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


def make_frames(fmt, h, w, t=T):
    return torch.from_numpy(C.random_frames(t, h, w, fmt, seed=11)).cuda()


def planes_of(frames, fmt):
    from pwstablenet_amd import stream as S
    return (S.window_planes_yuv if C.dtype(fmt) == np.uint8 else S.window_planes_yuv16)(frames, fmt)


def resize_of(frames, fmt, size):
    from pwstablenet_amd import stream as S
    return (S.area_resize_yuv if C.dtype(fmt) == np.uint8 else S.area_resize_yuv16)(frames, fmt, size)


def fields_of(vs, frames, fmt):
    fields = torch.empty((frames.shape[0], 256, 256, 2), device="cuda")
    with torch.no_grad():
        vs._fields(planes_of(frames, fmt), 0, 0, fields)
    return fields


def crop_by_hand(full, fmt, x0, x1, y0, y1):
    """The window of every plane, packed again (chroma_ref's packing)."""
    y, u, v = C.unpack(full.cpu().numpy(), fmt)
    cx, cy = C.shifts(fmt)
    c = lambda p: p[:, y0 >> cy:y1 >> cy, x0 >> cx:x1 >> cx]   # noqa: E731
    return torch.from_numpy(C.pack(y[:, y0:y1, x0:x1], c(u), c(v), fmt)).cuda()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", NAMES)
def test_run_selects_the_direct_warp(net, small, fmt, mode):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.stream import VideoStabilizer
    gray, fields = small
    frames = make_frames(fmt, 38, 52)
    vs = VideoStabilizer(net, batch=16, swap_rb=True, interpolation=mode)
    want = PF.upsample_grid_sample_yuv(frames, fields, fmt, align_corners=vs.align_corners, mode=mode)
    got = vs.run(gray, frames, pixel_format=fmt)
    assert got.shape == frames.shape and got.dtype == frames.dtype and got.is_cuda
    assert torch.equal(got, want)
    assert not torch.equal(got, frames)   # (the field moves the picture: the equality above compares warps, not copies)
    keep = VideoStabilizer(net, batch=16, swap_rb=True, interpolation=mode, borders="keep").run(gray, frames, pixel_format=fmt)
    kept = PF.keep_borders_(want.clone(), fields, frames[0], fmt, initial_is_source=True, align_corners=vs.align_corners, mode=mode)
    assert torch.equal(keep, kept)
    host = vs.run(gray.cpu(), frames.cpu().pin_memory(), pixel_format=fmt)   # host input: the same frames, on the host
    assert not host.is_cuda and torch.equal(host.cuda(), want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", NAMES)
def test_run_video_resize_and_crop(net, fmt, mode):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    h, w, size = 258, 260, (130, 128)
    four22 = C.ALL[fmt][2] == 1
    crop = (2, 24, 3, 16) if four22 else (3, 24, 3, 16)   # (x0, x1, y0, y1): an odd y edge; at 4:4:4 an odd x edge too
    frames = make_frames(fmt, h, w)
    vs = S.VideoStabilizer(net, batch=16, swap_rb=True, interpolation=mode)
    fields = fields_of(vs, frames, fmt)
    full = PF.upsample_grid_sample_yuv(frames, fields, fmt, align_corners=vs.align_corners, mode=mode)
    assert torch.equal(vs.run_video(frames, chunk=16, pixel_format=fmt), full)
    assert torch.equal(vs.run_video(frames, chunk=16, pixel_format=fmt, output_size=size), resize_of(full, fmt, size))
    cropped = vs.run_video(frames, chunk=16, pixel_format=fmt, crop=crop)
    assert cropped.shape == (T, C.packed_rows(fmt, 13), crop[1] - crop[0])
    assert torch.equal(cropped, crop_by_hand(full, fmt, *crop))
    if four22:
        with pytest.raises(ValueError, match="must have edges that are multiples of 2 \\(x\\) and 1 \\(y\\)"):
            vs.run_video(frames, chunk=16, pixel_format=fmt, crop=(3, 24, 3, 16))
        with pytest.raises(ValueError, match="output size 129 x 128 must be a multiple of 2 x 1"):
            vs.run_video(frames, chunk=16, pixel_format=fmt, output_size=(129, 128))
        odd = (130, 127)
    else:
        odd = (129, 127)
    assert torch.equal(vs.run_video(frames, chunk=16, pixel_format=fmt, output_size=odd), resize_of(full, fmt, odd))   # sizes 4:2:0 cannot have
    with pytest.raises(ValueError, match="frames_are_rgb has no meaning"):
        vs.run_video(frames, pixel_format=fmt, frames_are_rgb=True)


def test_in_flight_two_gives_the_same_frames(net):
    from pwstablenet_amd import stream as S
    fmt = "i422"
    frames = make_frames(fmt, 258, 260, t=6)
    vs = S.VideoStabilizer(net, batch=16, borders="keep")
    one = vs.run_video(frames, chunk=2, in_flight=1, pixel_format=fmt)
    two = vs.run_video(frames, chunk=2, in_flight=2, pixel_format=fmt)
    assert torch.equal(one, two) and not torch.equal(one, frames)
    host = vs.run_video(frames.cpu().pin_memory(), chunk=2, in_flight=2, pixel_format=fmt)
    assert not host.is_cuda and torch.equal(host.cuda(), one)


def test_zoom_is_zoom_fields_then_the_direct_warp(net):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    fmt, h, w = "p210", 258, 260
    frames = make_frames(fmt, h, w)
    vs = S.VideoStabilizer(net, batch=16)
    got = vs.run_video(frames, chunk=16, zoom=0.8, pixel_format=fmt)
    assert np.allclose(vs.zoom_windows, [(0.1 * w, 0.9 * w, 0.1 * h, 0.9 * h)] * T, rtol=0, atol=1e-9)
    zf = PF.zoom_fields(fields_of(vs, frames, fmt), vs.zoom_windows, (h, w), align_corners=vs.align_corners, mode=vs.interpolation)
    want = PF.upsample_grid_sample_yuv(frames, zf, fmt, align_corners=vs.align_corners, mode=vs.interpolation)
    assert got.shape == frames.shape and torch.equal(got, want)
    assert not torch.equal(got, vs.run_video(frames, chunk=16, pixel_format=fmt))


@pytest.mark.parametrize("fmt", ("nv16", "i410"))
def test_crop_auto_rounds_inward_to_the_format_s_multiples(hip, fmt):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    n, h, w = 34, 304, 600
    # zoomed out: black wedges on every side.  The shift is the first of a few that gives the BGR path's window an odd x edge AND an odd y
    # edge (4:2:0 would move both; 4:2:2 moves x alone, 4:4:4 neither): a test of the rounding needs something to round
    for shift in ((0.021, -0.013), (0.024, -0.016), (0.027, -0.019), (0.03, -0.022), (0.033, -0.025), (0.036, -0.028)):
        stub = _AffineStub(1.09, shift)
        _, bounds = S.field_homography(stub(torch.zeros((n, 31, 256, 256), device="cuda"), False), (h, w))
        x0, x1, y0, y1 = (int(v) for v in S.auto_crop_window(bounds, (h, w), (h, w), 30))
        print("%s, shift %s: the BGR path's window x [%d, %d) y [%d, %d)" % (fmt, shift, x0, x1, y0, y1))
        if (x0 | x1) & 1 and (y0 | y1) & 1:
            break
    else:
        raise AssertionError("none of the stand-ins gives a window with odd x and y edges")
    vs = S.VideoStabilizer(stub, batch=8)
    assert vs.period == 30
    frames = make_frames(fmt, h, w, t=n)
    assert 0 < x0 < x1 < w and 0 < y0 < y1 < h
    mx, my = PF.lookup_format(fmt).multiples
    window = (x0 + (-x0) % mx, x1 - x1 % mx, y0 + (-y0) % my, y1 - y1 % my)
    assert window == ((x0 + 1) // 2 * 2, x1 // 2 * 2, y0, y1) if fmt == "nv16" else window == (x0, x1, y0, y1)
    got = vs.run_video(frames, chunk=16, crop="auto", pixel_format=fmt)
    assert got.shape == (n, C.packed_rows(fmt, window[3] - window[2]), window[1] - window[0])
    assert torch.equal(got, vs.run_video(frames, chunk=16, crop=window, pixel_format=fmt))
