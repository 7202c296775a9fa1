"""GPU tests of VideoStabilizer(borders="mosaic"): run_video's chunk pipeline (a chunk finished one chunk late, its donors the last frames
of the chunk before it and the first of the chunk after it, cut at scene limits, applied before the output resize and the crop) against ONE
functional.mosaic_borders_ call per scene over the whole clip's "black" warp stage, bit for bit.

The clip is 20 frames of 288 x 320 (the smallest size the stabiliser takes: tests/test_hip_keep_stream.py), chunk = 8 (chunks of 8, 8 and 4
frames: the last one shorter than two radii), mosaic_radius = 3; the generator is test_hip_keep_stream.py's -- ngf = 16, synth's W1 weights with
the translation nudged so that a wedge opens on two sides."""
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

T, H, W, CHUNK, RADIUS, CUT = 20, 288, 320, 8, 3, 11


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
    y = synth.smooth_frames_u8(1, T, H, W, 21)[0]
    rs = np.random.RandomState(4)
    bgr = np.clip(np.stack([y * 0.9, y * 1.0, y * 0.8], -1) + rs.randint(-3, 4, (T, H, W, 3)), 0, 255).astype(np.uint8)
    _, u, v = R.unpack(R.random_yuv(T, H, W, "i420", seed=3), "i420")
    nv12 = R.pack(y, u, v, "nv12")
    p010 = R16.expand(nv12, "p010")
    return {"bgr24": torch.from_numpy(bgr).cuda(), "nv12": torch.from_numpy(nv12).cuda(), "p010": torch.from_numpy(p010).cuda()}


def eq(a, b):
    if a.dtype == torch.uint16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.shape == b.shape and torch.equal(a, b)


def planes_of(src, fmt):
    from pwstablenet_amd import stream as S
    return S.window_planes(src) if fmt == "bgr24" else (S.window_planes_yuv16 if fmt == "p010" else S.window_planes_yuv)(src, fmt)


def clip_fields(vs, src, fmt, cuts, chunk=CHUNK):
    """The fields run_video(chunk=chunk) forms, bit for bit: the same window planes in the same generator calls."""
    gray = planes_of(src, fmt)
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    half = vs.period // 2
    with torch.no_grad():
        for cs in range(0, T, chunk):
            ce = min(T, cs + chunk)
            hl, hr = min(half, cs), min(half, T - ce)
            sc = [t - (cs - hl) for t in cuts if cs - hl < t < ce + hr] or None
            vs._fields(gray[cs - hl:ce + hr], hl, hr, fields[cs:ce], sc)
    return fields


def fill_per_scene(warped, fields, fmt, cuts, kw):
    """One mosaic_borders_ call per scene over a copy of the black-border frames: (filled, unfilled)."""
    from pwstablenet_amd import functional as PF
    filled, counts = warped.clone(), []
    for a, b in zip([0] + list(cuts), list(cuts) + [warped.shape[0]]):
        counts.append(PF.mosaic_borders_(filled[a:b], fields[a:b], RADIUS, pixel_format=fmt, return_unfilled=True, **kw)[1])
    return filled, torch.cat(counts)


def expected(net, src, fmt, interpolation, cuts, swap_rb, chunk=CHUNK):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.stream import VideoStabilizer
    black = VideoStabilizer(net, batch=8, swap_rb=swap_rb, interpolation=interpolation, borders="black")
    warped = black.run_video(src, chunk=chunk, pixel_format=fmt, scene_cuts=cuts or None)
    assert black.mosaic_unfilled is None
    fields = clip_fields(black, src, fmt, cuts, chunk)
    kw = dict(align_corners=black.align_corners, mode=interpolation)
    if fmt == "bgr24":   # the fields are run_video's own: "black" is the plain warp of them, as it was
        assert eq(warped, PF.upsample_grid_sample_u8(src, fields, swap_rb=swap_rb, **kw))
    else:
        assert eq(warped, PF.upsample_grid_sample_yuv(src, fields, fmt, **kw))
    filled, unfilled = fill_per_scene(warped, fields, fmt, cuts, kw)
    return filled, unfilled, warped, fields


CASES = [
    # fmt, interpolation, on_host, cuts, half_size_output
    ("bgr24", "bilinear", False, [], False),
    ("bgr24", "bilinear", True, [CUT], False),
    ("bgr24", "bicubic", False, [CUT], True),
    ("nv12", "bilinear", True, [], False),
    ("nv12", "bicubic", False, [CUT], True),
    ("p010", "bilinear", False, [CUT], False),
    ("p010", "bilinear", True, [], True),
]


@pytest.mark.parametrize("fmt,interpolation,on_host,cuts,half", CASES)
def test_run_video_mosaic_equals_one_call_per_scene(hip, net, clips, fmt, interpolation, on_host, cuts, half):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    src = clips[fmt]
    swap = fmt == "bgr24"
    filled, unfilled, warped, _ = expected(net, src, fmt, interpolation, cuts, swap)
    assert not eq(filled, warped)   # (not vacuous: the pass changes the frames)
    want = S._output_resize(filled, PF.lookup_format(fmt), (W // 2, H // 2), True) if half else filled
    vs = S.VideoStabilizer(net, batch=8, swap_rb=swap, interpolation=interpolation, borders="mosaic", mosaic_radius=RADIUS)
    feed = src.cpu().pin_memory() if on_host else src
    got = vs.run_video(feed, chunk=CHUNK, pixel_format=fmt, scene_cuts=cuts or None, half_size_output=half)
    torch.cuda.synchronize()
    assert got.is_cuda != on_host and got.dtype == src.dtype
    assert eq(got.cuda(), want)
    assert vs.mosaic_unfilled.is_cuda and vs.mosaic_unfilled.dtype == torch.int32 and torch.equal(vs.mosaic_unfilled, unfilled)
    # Chunking does not change a byte of the pass: one chunk of 20 frames is the rule on that run's own "black" frames, and where the
    # generator's calls are the same -- no cut: batches of 8, 8 and 4 frames either way; a cut inside a chunk regroups them -- the same
    # bytes as chunk = 8.
    whole = vs.run_video(feed, chunk=T, pixel_format=fmt, scene_cuts=cuts or None, half_size_output=half)
    torch.cuda.synchronize()
    filled_t, unfilled_t, warped_t, _ = expected(net, src, fmt, interpolation, cuts, swap, chunk=T)
    want_t = S._output_resize(filled_t, PF.lookup_format(fmt), (W // 2, H // 2), True) if half else filled_t
    assert eq(whole.cuda(), want_t) and torch.equal(vs.mosaic_unfilled, unfilled_t)
    if not cuts:
        assert eq(warped_t, warped)
    if eq(warped_t, warped):
        assert eq(whole, got) and torch.equal(unfilled_t, unfilled)


def test_the_clip_has_wedges_that_get_filled(hip, net, clips):
    """Not vacuous: by the float64 restatement at least 1 % of the clip's pixels are uncovered, some of them find a donor and some do not."""
    filled, unfilled, warped, fields = expected(net, clips["bgr24"], "bgr24", "bilinear", [CUT], True)
    from pwstablenet_amd.stream import VideoStabilizer
    cov, dist = K.coverage(fields[::4].cpu().numpy(), H, W, VideoStabilizer(net).align_corners, 0)
    share = 1 - cov.mean()
    print("uncovered share of the clip: %.4f, unfilled per frame: %s" % (share, unfilled.tolist()))
    assert share >= 0.01
    changed = (filled != warped).any(-1).flatten(1).sum(1)
    assert (changed > 0).any() and unfilled.sum() > 0
    # only uncovered pixels change (a pixel within 0.01 of a threshold may be decided either way by the fp32 coordinate)
    assert ((filled != warped).any(-1)[::4].cpu().numpy() <= (~cov | (dist <= 1e-2))).all()


def test_auto_cuts_and_an_explicit_crop(hip, net, clips):
    """scene_cuts="auto" on a clip with a hard cut, an explicit crop and output_size: the same rule after the same resize and crop."""
    from pwstablenet_amd import stream as S
    src = clips["bgr24"].clone()
    src[CUT:] = 255 - src[CUT:].flip(1)   # a hard cut
    black = S.VideoStabilizer(net, batch=8, borders="black")
    warped = black.run_video(src, chunk=CHUNK, scene_cuts="auto", scene_min_len=4)
    cuts = list(black.scene_cuts)
    assert CUT in cuts
    fields = clip_fields(black, src, "bgr24", cuts)
    filled, unfilled = fill_per_scene(warped, fields, "bgr24", cuts, dict(align_corners=black.align_corners, mode="bilinear"))
    vs = S.VideoStabilizer(net, batch=8, borders="mosaic", mosaic_radius=RADIUS)
    got = vs.run_video(src, chunk=CHUNK, scene_cuts="auto", scene_min_len=4, output_size=(W // 2, H // 2), crop=(10, 150, 20, 130))
    assert vs.scene_cuts == cuts and torch.equal(vs.mosaic_unfilled, unfilled)
    assert eq(got, S.area_resize(filled, (W // 2, H // 2))[:, 20:130, 10:150].contiguous())


def test_run_alone(hip, net, clips):
    """run() fills from its own frames only: the whole clip in one call, cut at a scene limit; a shard's halo frames are no donors."""
    from pwstablenet_amd import stream as S
    src = clips["bgr24"]
    gray = planes_of(src, "bgr24")
    black = S.VideoStabilizer(net, batch=8, borders="black")
    vs = S.VideoStabilizer(net, batch=8, borders="mosaic", mosaic_radius=RADIUS)
    kw = dict(align_corners=vs.align_corners, mode="bilinear")
    for cuts in ([], [CUT]):
        warped = black.run(gray, src, scene_cuts=cuts or None)
        fields = torch.empty((T, 256, 256, 2), device="cuda")
        with torch.no_grad():
            black._fields(gray, 0, 0, fields, cuts or None)
        filled, unfilled = fill_per_scene(warped, fields, "bgr24", cuts, kw)
        assert not eq(filled, warped)
        got = vs.run(gray, src, scene_cuts=cuts or None)
        assert eq(got, filled) and torch.equal(vs.mosaic_unfilled, unfilled)
        host = vs.run(gray, src.cpu().pin_memory(), scene_cuts=cuts or None)
        assert not host.is_cuda and eq(host.cuda(), filled)
    # a shard: frames 6 .. 13 with halos of 6 -- the rule on those 8 frames alone
    warped = black.run(gray, src[6:14], halo_left=6, halo_right=6)
    fields = torch.empty((8, 256, 256, 2), device="cuda")
    with torch.no_grad():
        black._fields(gray, 6, 6, fields, None)
    filled, unfilled = fill_per_scene(warped, fields, "bgr24", [], kw)
    assert eq(vs.run(gray, src[6:14], halo_left=6, halo_right=6), filled) and torch.equal(vs.mosaic_unfilled, unfilled)
    assert black.run(gray, src).shape == src.shape and black.mosaic_unfilled is None


def test_black_and_keep_are_what_they_were(hip, net, clips):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    src = clips["nv12"]
    black = S.VideoStabilizer(net, batch=8)
    assert black.borders == "black" and black.mosaic_radius == 8
    warped = black.run_video(src, chunk=CHUNK, pixel_format="nv12", scene_cuts=[CUT])
    fields = clip_fields(black, src, "nv12", [CUT])
    kw = dict(align_corners=black.align_corners, mode="bilinear")
    assert eq(warped, PF.upsample_grid_sample_yuv420(src, fields, "nv12", **kw))
    kept = warped.clone()
    for a, b in ((0, CUT), (CUT, T)):
        PF.keep_borders_(kept[a:b], fields[a:b], src[a], "nv12", initial_is_source=True, **kw)
    keep = S.VideoStabilizer(net, batch=8, borders="keep")
    for in_flight in (1, 2):
        assert eq(keep.run_video(src, chunk=CHUNK, pixel_format="nv12", scene_cuts=[CUT], in_flight=in_flight), kept)
    assert keep.mosaic_unfilled is None and black.mosaic_unfilled is None


def test_the_errors(hip, net, clips):
    from pwstablenet_amd import stream as S
    src = clips["bgr24"]
    for r in (0, 16, -1):
        with pytest.raises(ValueError, match="mosaic_radius"):
            S.VideoStabilizer(net, borders="mosaic", mosaic_radius=r)
    assert S.VideoStabilizer(net, borders="mosaic").mosaic_radius == 8 and S.VideoStabilizer(net, borders="mosaic", mosaic_radius=15).mosaic_radius == 15
    vs = S.VideoStabilizer(net, batch=8, borders="mosaic", mosaic_radius=RADIUS)
    big = torch.zeros((4, 320, 640, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="crop"):        # one removes the wedges, the other fills them
        vs.run_video(big, crop="auto")
    for zoom in (0.9, "auto"):
        with pytest.raises(ValueError, match="zoom"):
            vs.run_video(big, zoom=zoom)
    with pytest.raises(ValueError, match="zoom"):
        vs.run(torch.zeros((4, 256, 256), device="cuda"), big, zoom=(10, 600, 10, 300))
    with pytest.raises(ValueError, match="in_flight"):   # the one-chunk delay across two lanes: the named follow-up
        vs.run_video(src, chunk=CHUNK, in_flight=2)
    with pytest.raises(ValueError, match="chunk"):       # adjacent chunks must suffice
        vs.run_video(src, chunk=RADIUS - 1)
    with pytest.raises(ValueError, match="integer pixel formats"):   # float frames
        vs.run(torch.zeros((4, 256, 256), device="cuda"), torch.zeros((4, 3, 64, 96), device="cuda"))
    assert vs.run_video(src[:RADIUS], chunk=RADIUS).shape == src[:RADIUS].shape   # chunk == radius is fine
