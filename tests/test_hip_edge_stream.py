"""GPU tests of VideoStabilizer(edge="clamp" | "mirror"): run_video's chunk pipeline -- the pass right behind every batch's warp, from the
batch's own source frames and the field that warped (after rigidity and zoom), before the output resize and the crop, and with
borders="mosaic" before the mosaic fill -- against ONE functional.edge_borders_ call over the whole clip's "pad" frames, bit for bit.

The clip is 24 frames of 288 x 320 (the smallest size the stabiliser takes: tests/test_hip_keep_stream.py), chunk = 8; the rigidity case
takes 12 frames of 304 x 608 (the homography fit's lattice needs 600 x 300).  The generator is test_hip_keep_stream.py's -- ngf = 16, synth's
W1 weights with the translation nudged so that a wedge opens on two sides."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chroma_ref  # noqa: E402
import keep_ref as K  # noqa: E402
import yuv16_ref as R16  # noqa: E402
import yuv_ref as R  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402

T, H, W, CHUNK, CUT = 24, 288, 320, 8, 11
TB, HB, WB = 12, 304, 608


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


def make_clips(t, h, w):
    y = synth.smooth_frames_u8(1, t, h, w, 21)[0]
    rs = np.random.RandomState(4)
    bgr = np.clip(np.stack([y * 0.9, y * 1.0, y * 0.8], -1) + rs.randint(-3, 4, (t, h, w, 3)), 0, 255).astype(np.uint8)
    _, u, v = R.unpack(R.random_yuv(t, h, w, "i420", seed=3), "i420")
    nv12 = R.pack(y, u, v, "nv12")
    p010 = R16.expand(nv12, "p010") | np.uint16(5)   # junk in the low bits: the read rule drops it
    i444 = chroma_ref.from420(R.pack(y, u, v, "i420"), "i420", "i444")
    return {k: torch.from_numpy(a).cuda() for k, a in (("bgr24", bgr), ("nv12", nv12), ("p010", p010), ("i444", i444))}


@pytest.fixture(scope="module")
def clips():
    return make_clips(T, H, W)


@pytest.fixture(scope="module")
def big_clip():
    return make_clips(TB, HB, WB)["bgr24"]


def eq(a, b):
    if a.dtype == torch.uint16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.shape == b.shape and torch.equal(a, b)


def clip_fields(vs, src, fmt, cuts, chunk=CHUNK):
    """The fields run_video(chunk=chunk) forms, bit for bit: the same window planes in the same generator calls (``_fields``)."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    t = src.shape[0]
    gray = S._window_planes(src, PF.lookup_format(fmt), 256, None, "test")
    fields = torch.empty((t, 256, 256, 2), device="cuda")
    half = vs.period // 2
    with torch.no_grad():
        for cs in range(0, t, chunk):
            ce = min(t, cs + chunk)
            hl, hr = min(half, cs), min(half, t - ce)
            sc = [c - (cs - hl) for c in cuts if cs - hl < c < ce + hr] or None
            vs._fields(gray[cs - hl:ce + hr], hl, hr, fields[cs:ce], sc)
    return fields


def finish(frames, fmt, output_size, crop):
    """run_video's output resize and crop."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    rec = PF.lookup_format(fmt)
    h, w = rec.frame_shape(frames)[1:]
    if output_size is not None:
        frames = S._output_resize(frames, rec, output_size, False)
        w, h = output_size
    if crop is not None:
        x0, x1, y0, y1 = crop
        frames = S._crop(frames, rec, h, w, y0, y1, x0, x1)
    return frames


def expected(net, src, fmt, interpolation, edge, cuts=(), swap_rb=False, rigidity=0.0, zoom=None, output_size=None, crop=None):
    """The same stabiliser's "pad" frames at full size, one edge_borders_ call over the whole clip with ``_fields``' fields (after rigidity
    and zoom, as they warped), then the resize and the crop: (expected output, pad frames, edge-filled frames, fields)."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    cuts = list(cuts)
    pad = S.VideoStabilizer(net, batch=8, swap_rb=swap_rb, interpolation=interpolation, rigidity=rigidity)
    assert pad.edge == "pad"
    warped = pad.run_video(src, chunk=CHUNK, pixel_format=fmt, scene_cuts=cuts or None, zoom=zoom)
    rec = PF.lookup_format(fmt)
    hw = rec.frame_shape(src)[1:]
    fields = clip_fields(pad, src, fmt, cuts)
    if rigidity:
        fields = PF.rigid_fields(fields, S.field_homography(fields, hw)[0], hw, rigidity)
    if zoom is not None:
        fields = PF.zoom_fields(fields, pad.zoom_windows, hw, align_corners=pad.align_corners, mode=interpolation)
    kw = dict(swap_rb=swap_rb, align_corners=pad.align_corners, mode=interpolation)
    assert eq(warped, PF.warp(src, fields, rec, **kw))   # the fields are the ones that warped: "pad" comes out of them bit for bit
    filled = PF.edge_borders_(warped.clone(), src, fields, edge, fmt, **kw)
    return finish(filled, fmt, output_size, crop), warped, filled, fields


def test_the_clip_uncovers_a_wedge_and_the_pass_fills_it(hip, net, clips):
    """Not vacuous: by the float64 restatement at least 1 % of the pixels are uncovered (every 8th frame is counted); "pad" paints most of
    them black, an edge mode next to none."""
    from pwstablenet_amd.stream import VideoStabilizer
    for edge in ("clamp", "mirror"):
        _, warped, filled, fields = expected(net, clips["bgr24"], "bgr24", "bilinear", edge, swap_rb=True)
        cov, _ = K.coverage(fields[::8].cpu().numpy(), H, W, VideoStabilizer(net).align_corners, 0)
        assert 1 - cov.mean() >= 0.01
        wedge = torch.from_numpy(~cov).cuda()
        assert not eq(filled, warped)
        assert (warped[::8][wedge] == 0).float().mean() > 0.5 and (filled[::8][wedge] == 0).float().mean() < 0.05
        assert eq(filled[::8][~wedge], warped[::8][~wedge])


CASES = [
    # fmt, interpolation, edge, swap_rb, in_flight, on_host, cuts, output_size, crop, zoom
    ("bgr24", "bilinear", "mirror", True, 1, False, [], None, None, None),
    ("bgr24", "bilinear", "clamp", False, 2, True, [], None, None, None),
    ("bgr24", "bicubic", "mirror", True, 2, False, [CUT], None, None, None),
    ("bgr24", "bilinear", "clamp", True, 1, True, [], (W // 2, H // 2), None, None),
    ("bgr24", "bicubic", "clamp", False, 1, False, [], None, (10, 300, 20, 260), None),
    ("bgr24", "bilinear", "mirror", False, 2, False, [], None, None, 0.9),
    ("nv12", "bilinear", "clamp", False, 2, False, [CUT], None, None, None),
    ("nv12", "bicubic", "mirror", False, 1, True, [], (W // 2, H // 2), (10, 150, 20, 130), None),
    ("p010", "bilinear", "mirror", False, 2, False, [], None, None, None),
    ("p010", "bicubic", "clamp", False, 1, False, [CUT], None, None, 0.9),
    ("i444", "bilinear", "clamp", False, 1, False, [CUT], None, None, None),
    ("i444", "bicubic", "mirror", False, 2, True, [], None, (11, 301, 21, 261), None),
]


@pytest.mark.parametrize("fmt,interpolation,edge,swap,in_flight,on_host,cuts,output_size,crop,zoom", CASES)
def test_run_video_edge_equals_one_call_over_the_clip(hip, net, clips, fmt, interpolation, edge, swap, in_flight, on_host, cuts, output_size, crop, zoom):
    from pwstablenet_amd.stream import VideoStabilizer
    src = clips[fmt]
    want, warped, filled, _ = expected(net, src, fmt, interpolation, edge, cuts, swap, 0.0, zoom, output_size, crop)
    if zoom is None:   # (a zoom of 0.9 leaves little of the wedge; without one the pass changes the frames)
        assert not eq(filled, warped)
    vs = VideoStabilizer(net, batch=8, swap_rb=swap, interpolation=interpolation, edge=edge)
    feed = src.cpu().pin_memory() if on_host else src
    got = vs.run_video(feed, chunk=CHUNK, in_flight=in_flight, pixel_format=fmt, scene_cuts=cuts or None, output_size=output_size, crop=crop, zoom=zoom)
    torch.cuda.synchronize()
    assert got.is_cuda != on_host and got.dtype == src.dtype
    assert eq(got.cuda(), want)
    other = vs.run_video(src, chunk=CHUNK, in_flight=3 - in_flight, pixel_format=fmt, scene_cuts=cuts or None, output_size=output_size, crop=crop, zoom=zoom)
    assert eq(other, want)   # in_flight = 2 equals in_flight = 1


def test_rigidity(hip, net, big_clip):
    from pwstablenet_amd.stream import VideoStabilizer
    for edge, interpolation in (("mirror", "bilinear"), ("clamp", "bicubic")):
        want, warped, filled, _ = expected(net, big_clip, "bgr24", interpolation, edge, rigidity=0.6)
        assert not eq(filled, warped)
        vs = VideoStabilizer(net, batch=8, interpolation=interpolation, rigidity=0.6, edge=edge)
        assert eq(vs.run_video(big_clip, chunk=CHUNK, in_flight=2), want)


def test_automatic_crop_and_zoom(hip, net, big_clip):
    """The two-pass paths run the pass behind their own warp: the frames are those of the explicit window / the windows they chose."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    vs = S.VideoStabilizer(net, batch=8, edge="mirror")
    pad = S.VideoStabilizer(net, batch=8)
    got = vs.run_video(big_clip, chunk=CHUNK, zoom="auto")
    fields = PF.zoom_fields(clip_fields(pad, big_clip, "bgr24", []), vs.zoom_windows, (HB, WB), align_corners=pad.align_corners)
    black = pad.run_video(big_clip, chunk=CHUNK, zoom="auto")
    assert eq(black, PF.warp(big_clip, fields, PF.lookup_format("bgr24"), align_corners=pad.align_corners))
    assert eq(got, PF.edge_borders_(black.clone(), big_clip, fields, "mirror", align_corners=pad.align_corners))
    auto = vs.run_video(big_clip, chunk=CHUNK, crop="auto")
    bounds = S.field_homography(clip_fields(pad, big_clip, "bgr24", []), (HB, WB))[1]
    window = S.auto_crop_window(bounds, (HB, WB), (HB, WB), vs.period)
    assert eq(auto, vs.run_video(big_clip, chunk=CHUNK, crop=window))      # crop="auto" is the single pass with the window it chose
    assert not eq(auto, pad.run_video(big_clip, chunk=CHUNK, crop="auto"))   # and its second pass ran the edge pass


def test_a_shard_with_halos_equals_the_unsharded_clip(hip, net, clips):
    """Nothing crosses a frame, so a shard needs no history: its bytes are the unsharded clip's wherever its fields are.  The generator's
    output depends on how frames are batched in the last bit ("pad" itself is held to 1 LSB across shards in tests/test_hip_stream.py), so
    the shards here begin and end where the unsharded clip's batches of 8 do: the same generator calls, the same fields, the same bytes --
    unlike "keep" and "mosaic", which do not promise them even then."""
    from pwstablenet_amd.stream import VideoStabilizer
    for fmt, edge in (("bgr24", "mirror"), ("nv12", "clamp")):
        src = clips[fmt]
        vs = VideoStabilizer(net, batch=8, edge=edge)
        whole = vs.run_video(src, chunk=CHUNK, pixel_format=fmt)
        assert not eq(whole, VideoStabilizer(net, batch=8).run_video(src, chunk=CHUNK, pixel_format=fmt))
        half = vs.period // 2
        for a, b in ((8, 16), (16, 24), (8, 24)):          # frames [a, b) with every real neighbour the windows reach
            hl, hr = min(half, a), min(half, T - b)
            shard = vs.run_video(src[a - hl:b + hr], chunk=CHUNK, pixel_format=fmt, halo_left=hl, halo_right=hr)
            assert eq(shard, whole[a:b]), (fmt, a, b)


@pytest.mark.parametrize("fmt,interpolation,edge,cuts", [("bgr24", "bilinear", "mirror", []), ("nv12", "bicubic", "clamp", [CUT]),
                                                          ("p010", "bilinear", "clamp", [])])
def test_mosaic_shows_the_edge_fill_exactly_where_it_finds_no_donor(hip, net, clips, fmt, interpolation, edge, cuts):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    R = 3
    src, swap = clips[fmt], fmt == "bgr24"
    _, warped, filled, fields = expected(net, src, fmt, interpolation, edge, cuts, swap)
    kw = dict(pixel_format=fmt, align_corners=S.VideoStabilizer(net).align_corners, mode=interpolation, return_unfilled=True)
    want, plain, counts = filled.clone(), warped.clone(), []
    for a, b in zip([0] + cuts, cuts + [T]):   # one mosaic call per scene, over the edge-filled and over the plain black frames
        PF.mosaic_borders_(want[a:b], fields[a:b], R, **kw)
        counts.append(PF.mosaic_borders_(plain[a:b], fields[a:b], R, **kw)[1])
    counts = torch.cat(counts)
    vs = S.VideoStabilizer(net, batch=8, swap_rb=swap, interpolation=interpolation, borders="mosaic", mosaic_radius=R, edge=edge)
    got = vs.run_video(src, chunk=CHUNK, pixel_format=fmt, scene_cuts=cuts or None)
    assert eq(got, want)
    assert torch.equal(vs.mosaic_unfilled, counts)   # mosaic_unfilled keeps its meaning
    ref = S.VideoStabilizer(net, batch=8, swap_rb=swap, interpolation=interpolation, borders="mosaic", mosaic_radius=R)
    assert eq(ref.run_video(src, chunk=CHUNK, pixel_format=fmt, scene_cuts=cuts or None), plain) and torch.equal(ref.mosaic_unfilled, counts)
    # it differs from plain mosaic only at positions plain mosaic left unfilled: there plain mosaic shows the black warp's sample, and the
    # edge-filled clip the edge fill's
    differs = (got != plain) if got.dtype != torch.uint16 else (got.view(torch.int16) != plain.view(torch.int16))
    pw, fw = (warped, filled) if got.dtype != torch.uint16 else (warped.view(torch.int16), filled.view(torch.int16))
    g, p = (got, plain) if got.dtype != torch.uint16 else (got.view(torch.int16), plain.view(torch.int16))
    assert differs.any() and counts.sum() > 0
    assert bool(((p == pw) & (g == fw))[differs].all())
    # and the Y (BGR: pixel) positions that differ are no more than the unfilled count of their frame
    ypos = differs[:, :H].reshape(T, -1) if fmt != "bgr24" else differs.any(-1).reshape(T, -1)
    assert bool((ypos.sum(1) <= counts).all())


def test_pad_is_the_default_and_the_errors(hip, net, clips):
    from pwstablenet_amd import stream as S
    src = clips["bgr24"]
    default, pad = S.VideoStabilizer(net, batch=8), S.VideoStabilizer(net, batch=8, edge="pad")
    assert default.edge == "pad" and pad.edge == "pad"
    assert eq(default.run_video(src, chunk=CHUNK, in_flight=2), pad.run_video(src, chunk=CHUNK, in_flight=2))
    for bad in ("wrap", "black", None, 1):
        with pytest.raises(ValueError, match="edge"):
            S.VideoStabilizer(net, edge=bad)
    with pytest.raises(ValueError):
        S.VideoStabilizer(net, borders="mirror")          # the mode is no value of `borders`
    for edge in ("clamp", "mirror"):
        with pytest.raises(ValueError, match="keep"):
            S.VideoStabilizer(net, borders="keep", edge=edge)
    assert S.VideoStabilizer(net, borders="keep", edge="pad").edge == "pad"
    vs = S.VideoStabilizer(net, batch=8, edge="clamp")
    with pytest.raises(ValueError, match="integer pixel formats"):      # float frames
        vs.run(torch.zeros((4, 256, 256), device="cuda"), torch.zeros((4, 3, 64, 96), device="cuda"))
    assert pad.run(torch.zeros((4, 256, 256), device="cuda"), torch.zeros((4, 3, 64, 96), device="cuda")).shape == (4, 3, 64, 96)
