"""GPU tests of VideoStabilizer(borders="keep"): run_video's chunk pipeline (history carried from chunk to chunk and from lane to lane, reset
at scene cuts, applied before the output resize and the crop) against ONE functional.keep_borders_ call per scene over the whole clip's
"black" warp stage.

The clip is 40 frames of 288 x 320, not 64 x 96: run_video computes the 256 x 256 window planes itself and INTER_AREA refuses to up-scale, so
288 x 320 (tests/test_hip_scene_cuts.py's size) is the smallest clip the stabiliser takes.  The ngf = 16 generator carries synth's W1 weights
with the translation entries of ``linear``'s bias nudged by +0.10 / -0.08, which moves the picture by about 5 % / 4 % of the frame: a wedge
on two sides (asserted: at least 1 % of the pixels are uncovered)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keep_ref as K  # noqa: E402
import yuv16_ref as R16  # noqa: E402
import yuv_ref as R  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402

T, H, W, CHUNK = 40, 288, 320, 16


@pytest.fixture(scope="module")
def net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    weights = dict(synth.make_weights("W1", seed=123, ngf=16))
    bias = weights["linear.mpconv.0.bias"].copy()
    bias[2] += np.float32(0.10)
    bias[5] -= np.float32(0.08)
    weights["linear.mpconv.0.bias"] = bias
    g = define_G(31, 2, 16, "normal", 0.02)
    g.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in weights.items()})
    return g.cuda()


@pytest.fixture(scope="module")
def clips():
    """The clip in every format, on the device: smooth shaky luma (synth.smooth_frames_u8) under tinted channels / smooth chroma."""
    y = synth.smooth_frames_u8(1, T, H, W, 21)[0]
    rs = np.random.RandomState(4)
    bgr = np.clip(np.stack([y * 0.9, y * 1.0, y * 0.8], -1) + rs.randint(-3, 4, (T, H, W, 3)), 0, 255).astype(np.uint8)
    _, u, v = R.unpack(R.random_yuv(T, H, W, "i420", seed=3), "i420")
    nv12 = R.pack(y, u, v, "nv12")
    p010 = R16.expand(nv12, "p010") | np.uint16(5)   # junk in the low bits: the initial frame's read rule masks it
    return {"bgr24": torch.from_numpy(bgr).cuda(), "nv12": torch.from_numpy(nv12).cuda(), "p010": torch.from_numpy(p010).cuda()}


def eq(a, b):
    if a.dtype == torch.uint16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.shape == b.shape and torch.equal(a, b)


def clip_fields(vs, src, fmt, cuts):
    """The fields run_video(chunk=CHUNK) forms, bit for bit: the same window planes in the same generator calls (what crop="auto"'s first
    pass does)."""
    from pwstablenet_amd import stream as S
    gray = S.window_planes(src) if fmt == "bgr24" else (S.window_planes_yuv16 if fmt == "p010" else S.window_planes_yuv)(src, fmt)
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    half = vs.period // 2
    with torch.no_grad():
        for cs in range(0, T, CHUNK):
            ce = min(T, cs + CHUNK)
            hl, hr = min(half, cs), min(half, T - ce)
            sc = [t - (cs - hl) for t in cuts if cs - hl < t < ce + hr] or None
            vs._fields(gray[cs - hl:ce + hr], hl, hr, fields[cs:ce], sc)
    return fields


def finish(frames, fmt, output_size, crop):
    """run_video's output resize and crop."""
    from pwstablenet_amd import stream as S
    if output_size is not None:
        frames = S.area_resize(frames, output_size) if fmt == "bgr24" else (S.area_resize_yuv16 if fmt == "p010" else S.area_resize_yuv)(frames, fmt, output_size)
    if crop is not None:
        x0, x1, y0, y1 = crop
        if fmt == "bgr24":
            frames = frames[:, y0:y1, x0:x1].contiguous()
        else:
            oh = frames.shape[1] * 2 // 3
            frames = S._yuv_crop(frames, oh, frames.shape[2], fmt, y0, y1, x0, x1)
    return frames


def expected(net, src, fmt, interpolation, cuts, output_size, crop, swap_rb):
    """borders="black" at full size, keep_borders_ over the whole clip in one segment per scene, then the resize and the crop."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.stream import VideoStabilizer
    black = VideoStabilizer(net, batch=8, swap_rb=swap_rb, interpolation=interpolation, borders="black")
    warped = black.run_video(src, chunk=CHUNK, pixel_format=fmt, scene_cuts=cuts or None)
    fields = clip_fields(black, src, fmt, cuts)
    kw = dict(align_corners=black.align_corners, mode=interpolation)
    if fmt == "bgr24":   # the fields are run_video's own: the warp stage comes out of them bit for bit
        assert eq(warped, PF.upsample_grid_sample_u8(src, fields, swap_rb=swap_rb, **kw))
    elif fmt == "nv12":
        assert eq(warped, PF.upsample_grid_sample_yuv420(src, fields, fmt, **kw))
    else:
        assert eq(warped, PF.upsample_grid_sample_yuv420_16(src, fields, fmt, **kw))
    kept = warped.clone()
    for a, b in zip([0] + list(cuts), list(cuts) + [T]):
        PF.keep_borders_(kept[a:b], fields[a:b], src[a], fmt, initial_is_source=True, swap_rb=swap_rb, **kw)
    return finish(kept, fmt, output_size, crop), warped, kept, fields


def test_the_clip_uncovers_a_wedge(hip, net, clips):
    """Not vacuous: by the float64 restatement at least 1 % of the pixels of the clip's frames are uncovered (every 8th frame is counted),
    the pass changes the frames, and no kept frame shows the pad colour in the wedge that "black" paints."""
    want, warped, kept, fields = expected(net, clips["bgr24"], "bgr24", "bilinear", [], None, None, True)
    from pwstablenet_amd.stream import VideoStabilizer
    cov, _ = K.coverage(fields[::8].cpu().numpy(), H, W, VideoStabilizer(net).align_corners, 0)
    share = 1 - cov.mean()
    print("uncovered share of the clip: %.4f" % share)
    assert share >= 0.01
    assert not eq(kept, warped)
    wedge = torch.from_numpy(~cov).cuda()
    assert (warped[::8][wedge] == 0).float().mean() > 0.5 and (kept[::8][wedge] == 0).float().mean() < 0.05


CASES = [
    # fmt, interpolation, in_flight, on_host, cuts, output_size, crop
    ("bgr24", "bilinear", 1, False, [], None, None),
    ("bgr24", "bilinear", 2, False, [], None, None),
    ("bgr24", "bilinear", 1, True, [], None, None),
    ("bgr24", "bilinear", 2, True, [], None, None),
    ("bgr24", "bilinear", 1, False, [17], None, None),
    ("bgr24", "bilinear", 2, True, [17], None, None),
    ("bgr24", "bilinear", 2, False, [], (W // 2, H // 2), None),
    ("bgr24", "bilinear", 1, True, [], None, (10, 300, 20, 260)),
    ("bgr24", "bicubic", 2, False, [17], None, None),
    ("nv12", "bilinear", 2, False, [], None, None),
    ("nv12", "bilinear", 1, True, [17], (W // 2, H // 2), None),
    ("nv12", "bicubic", 2, True, [], None, (10, 300, 20, 260)),
    ("p010", "bilinear", 2, False, [17], None, None),
]


@pytest.mark.parametrize("fmt,interpolation,in_flight,on_host,cuts,output_size,crop", CASES)
def test_run_video_keep_equals_one_segment_per_scene(hip, net, clips, fmt, interpolation, in_flight, on_host, cuts, output_size, crop):
    from pwstablenet_amd.stream import VideoStabilizer
    src = clips[fmt]
    swap = fmt == "bgr24"
    want, warped, kept, _ = expected(net, src, fmt, interpolation, cuts, output_size, crop, swap)
    assert not eq(kept, warped)
    vs = VideoStabilizer(net, batch=8, swap_rb=swap, interpolation=interpolation, borders="keep")
    feed = src.cpu().pin_memory() if on_host else src
    got = vs.run_video(feed, chunk=CHUNK, in_flight=in_flight, pixel_format=fmt, scene_cuts=cuts or None, output_size=output_size, crop=crop)
    torch.cuda.synchronize()
    assert got.is_cuda != on_host and got.dtype == src.dtype
    assert eq(got.cuda(), want)


def test_half_size_output_and_run(hip, net, clips):
    """half_size_output is the pass before area_half; run() alone carries the history from batch to batch and through keep_from."""
    from pwstablenet_amd import stream as S
    src = clips["bgr24"]
    want, _, kept, _ = expected(net, src, "bgr24", "bilinear", [], None, None, False)
    vs = S.VideoStabilizer(net, batch=8, borders="keep")
    assert eq(vs.run_video(src, chunk=CHUNK, half_size_output=True), S.area_half(kept))
    gray = S.window_planes(src)
    whole = vs.run(gray[:CHUNK + 15], src[:CHUNK], halo_right=15)       # run_video's first chunk: two batches of 8
    assert eq(whole, kept[:CHUNK])
    nxt = vs.run(gray[1:CHUNK + 8 + 15], src[CHUNK:CHUNK + 8], halo_left=15, halo_right=15, keep_from=whole[-1])
    assert eq(nxt, kept[CHUNK:CHUNK + 8])
    alone = vs.run(gray[1:CHUNK + 8 + 15], src[CHUNK:CHUNK + 8], halo_left=15, halo_right=15)   # a shard: no history, starts from its source
    assert not eq(alone, nxt)


def test_black_is_the_default_and_the_errors(hip, net, clips):
    from pwstablenet_amd import stream as S
    src = clips["bgr24"]
    default, black = S.VideoStabilizer(net, batch=8), S.VideoStabilizer(net, batch=8, borders="black")
    assert default.borders == "black"
    assert eq(default.run_video(src, chunk=CHUNK, in_flight=2), black.run_video(src, chunk=CHUNK, in_flight=2))
    with pytest.raises(ValueError):
        S.VideoStabilizer(net, borders="mirror")
    keep = S.VideoStabilizer(net, batch=8, borders="keep")
    big = torch.zeros((4, 320, 640, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):      # one removes the wedges, the other fills them
        keep.run_video(big, crop="auto")
    with pytest.raises(ValueError):      # float frames
        keep.run(torch.zeros((4, 256, 256), device="cuda"), torch.zeros((4, 3, 64, 96), device="cuda"))
    assert black.run(torch.zeros((4, 256, 256), device="cuda"), torch.zeros((4, 3, 64, 96), device="cuda")).shape == (4, 3, 64, 96)
