"""GPU tests of the scene-cut support: pws_scene_change against the numpy restatement (tests/scene_ref.py) bit for bit, a scene of
VideoStabilizer.run(scene_cuts=...) against the clip made of that scene alone, run_video with explicit and detected cuts, and
crop="auto" across a cut."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_ref as R  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402

SEED_PAIRS = [(1, 2), (3, 4), (5, 6), (123, 321), (7, 8), (9, 10)]


@pytest.fixture(scope="module")
def net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    g = define_G(31, 2, 16, "normal", 0.02)
    g.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=16)})
    return g.cuda()


def _special_values():
    """the 33 bin edges k/16 - 1 with their fp32 neighbours on both sides, exactly -1 and +1, the infinities and NaN"""
    e = (np.arange(33, dtype=np.float32) / np.float32(16) - np.float32(1)).astype(np.float32)
    return np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf)),
                           np.array([-1.0, 1.0, np.inf, -np.inf, np.nan, -np.nan], np.float32)]).astype(np.float32)


def _inputs(n, h, w):
    rs = np.random.RandomState(n * 100 + h + w)
    smooth = synth.smooth_frames_u8(1, n, h, w, seed=h + w)[0]
    sp = _special_values()
    special = np.stack([np.roll(np.resize(sp, h * w), 7 * t).reshape(h, w) for t in range(n)])   # (rolled: the frames differ, sad > 0)
    return {"uniform": rs.uniform(-1.2, 1.2, (n, h, w)).astype(np.float32),
            "window": (smooth.astype(np.float32) / np.float32(255) * np.float32(2) - np.float32(1)).astype(np.float32),
            "special": special.astype(np.float32)}


# (1, 4, 4): one pixel per block; (2, 8, 12) and (3, 100, 36): block rows that are no multiple of 4 floats (scalar loads), 100 x 36 with more
# samples per block than threads; (5, 64, 64) and (2, 128, 64): float4 loads, fewer / more items than threads; (33, 256, 256): the live shape
@pytest.mark.parametrize("shape", [(1, 4, 4), (2, 8, 12), (3, 100, 36), (5, 64, 64), (33, 256, 256), (2, 128, 64)])
def test_counters_equal_the_restatement_bit_for_bit(hip, shape):
    from pwstablenet_amd.stream import scene_scores
    n, h, w = shape
    for name, planes in _inputs(n, h, w).items():
        d = torch.from_numpy(planes).cuda()
        scores, hist, sad = scene_scores(d, return_counts=True)
        assert hist.dtype == sad.dtype == torch.int32 and hist.shape == (n, 16, 32) and sad.shape == (n,)
        assert scores.dtype == torch.float32 and scores.shape == (n,) and scores.is_cuda
        want_h = R.hist(planes)
        assert int(want_h.sum()) == n * h * w
        assert np.array_equal(hist.cpu().numpy().astype(np.uint32), want_h), name
        assert np.array_equal(sad.cpu().numpy().astype(np.uint32), R.sad(want_h)), name
        assert int(sad[0]) == 0
        assert torch.equal(scores, sad.float() / (2 * h * w)), name
        # against numpy's division: torch divides a device tensor by a Python scalar as a product with the scalar's reciprocal, which is
        # the correctly rounded quotient when 2 h w is a power of two (the live 256 x 256 among them) and within one ulp of it otherwise
        if (2 * h * w) & (2 * h * w - 1) == 0:
            assert np.array_equal(scores.cpu().numpy(), R.scores(planes)), name
        else:
            np.testing.assert_array_max_ulp(scores.cpu().numpy(), R.scores(planes), maxulp=1)
        assert float(scores.min()) >= 0 and float(scores.max()) <= 1
        again = scene_scores(d, return_counts=True)
        assert all(torch.equal(a, b) for a, b in zip(again, (scores, hist, sad))), name
        assert torch.equal(scene_scores(d), scores)
    if n > 1:
        assert int(sad[1]) > 0


def test_special_samples_land_in_the_defined_bins(hip):
    from pwstablenet_amd.stream import scene_scores
    v = torch.tensor([-1.0, 1.0, float("inf"), float("-inf"), float("nan"), -1.0000001, 0.9999999, 0.0,
                      -0.0, -0.93750006, -0.9375, 5.0, -5.0, 0.0625, 0.99, -0.99]).view(1, 4, 4).cuda()
    _, hist, sad = scene_scores(v, return_counts=True)
    bins = hist[0].argmax(1).cpu().tolist()           # one pixel per block: its bin is the block's one non-zero counter
    assert hist[0].sum(1).cpu().tolist() == [1] * 16 and sad.cpu().tolist() == [0]
    assert bins == [0, 31, 31, 0, 0, 0, 31, 16, 16, 0, 1, 31, 0, 17, 31, 0]


def test_scene_scores_errors(hip):
    from pwstablenet_amd.stream import scene_scores
    x = torch.zeros((3, 8, 8), device="cuda")
    for bad in (x.transpose(1, 2)[:, :, ::2], x[:, ::2], x.double(), x.half(), x[0], x.to(torch.int32)):
        with pytest.raises(ValueError):
            scene_scores(bad)
    L = hip.lib()
    hist, sad = torch.zeros((3, 16, 32), dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    for h, w in ((6, 8), (8, 6), (7, 7)):
        assert L.pws_scene_change(hip.ptr(x), 3, h, w, hip.ptr(hist), hip.ptr(sad), None) == -22
        assert b"multiples of 4" in L.pws_last_error()
    assert L.pws_scene_change(None, 3, 8, 8, hip.ptr(hist), hip.ptr(sad), None) == -22 and b"NULL" in L.pws_last_error()
    assert L.pws_scene_change(None, 0, 8, 8, None, None, None) == 0
    with pytest.raises(RuntimeError, match="multiples of 4"):
        scene_scores(torch.zeros((2, 6, 8), device="cuda"))
    assert scene_scores(torch.zeros((0, 8, 8), device="cuda")).shape == (0,)


@pytest.fixture(scope="module")
def two_scenes():
    """34 window planes -- a scene of 21 and one of 13 frames -- and 34 fp32 frames, on the device"""
    gray = np.concatenate([synth.make_window(1, 21, 256, seed=4)[0], synth.make_window(1, 13, 256, seed=8)[0]])
    return torch.from_numpy(gray).cuda(), torch.from_numpy(synth.make_frames(34, 3, 72, 128, seed=5)).cuda()


def test_a_scene_equals_the_clip_of_that_scene(hip, net, two_scenes):
    from pwstablenet_amd.stream import VideoStabilizer
    gray, frames = two_scenes
    vs = VideoStabilizer(net, batch=4)
    plain = vs.run(gray, frames)
    cut = vs.run(gray, frames, scene_cuts=[21])
    assert torch.equal(cut, torch.cat([vs.run(gray[:21], frames[:21]), vs.run(gray[21:], frames[21:])]))
    # the clamp does something: every frame whose window crossed the cut changes
    for i in list(range(6, 34)):
        assert not torch.equal(cut[i], plain[i]), i
    assert torch.equal(cut[:4], plain[:4])            # (the first batch of the first scene never saw the cut)
    assert torch.equal(vs.run(gray, frames, scene_cuts=[]), plain)
    assert torch.equal(vs.run(gray, frames, scene_cuts=None), plain)
    # two cuts, the middle scene shorter than a window's half (and than min_scene)
    got = vs.run(gray, frames, scene_cuts=(15, 20))
    assert torch.equal(got, torch.cat([vs.run(gray[:15], frames[:15]), vs.run(gray[15:20], frames[15:20]), vs.run(gray[20:], frames[20:])]))
    # pinned-host inputs: the batches' uploads follow the scenes
    got_h = vs.run(gray.cpu().pin_memory(), frames.cpu().pin_memory(), scene_cuts=[21])
    assert not got_h.is_cuda and torch.equal(got_h, cut.cpu())


def test_a_scene_equals_the_clip_of_that_scene_with_halos(hip, net, two_scenes):
    from pwstablenet_amd.stream import VideoStabilizer
    gray, frames = two_scenes
    vs = VideoStabilizer(net, batch=4)
    core = frames[3:32]                               # halo_left 3, halo_right 2: 29 frames to stabilise, gray indices 3 .. 31
    # a cut inside the left halo: gray frames 0, 1 belong to a scene that holds nothing to stabilise
    got = vs.run(gray, core, halo_left=3, halo_right=2, scene_cuts=[2, 21])
    want = torch.cat([vs.run(gray[2:21], core[:18], halo_left=1, halo_right=0), vs.run(gray[21:], core[18:], halo_left=0, halo_right=2)])
    assert torch.equal(got, want)
    # ... and one inside the right halo as well
    got = vs.run(gray, core, halo_left=3, halo_right=2, scene_cuts=[2, 21, 33])
    want = torch.cat([vs.run(gray[2:21], core[:18], halo_left=1, halo_right=0), vs.run(gray[21:33], core[18:], halo_left=0, halo_right=1)])
    assert torch.equal(got, want)
    for bad in ([0], [34], [21, 21], [21, 5], [40]):
        with pytest.raises(ValueError):
            vs.run(gray, core, halo_left=3, halo_right=2, scene_cuts=bad)


def _clip_u8(T, H, W, seed):
    """A shaky clip as tests/test_hip_stream.py makes it: one smooth scene under small per-frame translations + a little sensor noise."""
    rs = np.random.RandomState(seed)
    base = synth.smooth_frames_u8(1, T, H, W, seed)[0]
    col = np.stack([base * 0.9, base * 1.0, base * 0.8], -1) + rs.randint(-3, 4, (T, H, W, 3))
    return np.clip(col, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def edited_clip():
    """48 frames of 288 x 320: a scene of 32 frames, then one of 16"""
    return torch.from_numpy(np.concatenate([_clip_u8(32, 288, 320, 11), _clip_u8(16, 288, 320, 12)]))


@pytest.mark.parametrize("on_host", [False, True])
@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("graph", [False, True])
def test_run_video_cut_on_the_chunk_grid(hip, net, edited_clip, on_host, in_flight, graph):
    from pwstablenet_amd.stream import VideoStabilizer
    src = edited_clip.pin_memory() if on_host else edited_clip.cuda()
    vs = VideoStabilizer(net, batch=8, swap_rb=True)
    net.module.enable_graph(graph)
    try:
        got = vs.run_video(src, chunk=16, in_flight=in_flight, scene_cuts=[32])
        want = torch.cat([vs.run_video(src[:32], chunk=16, in_flight=in_flight), vs.run_video(src[32:], chunk=16, in_flight=in_flight)])
        plain = vs.run_video(src, chunk=16, in_flight=in_flight)
        torch.cuda.synchronize()
    finally:
        net.module.enable_graph(False)
    assert got.is_cuda != on_host and got.dtype == torch.uint8 and vs.scene_cuts == []     # (of the last call, which had none)
    assert torch.equal(got, want)
    assert not torch.equal(got[17:47], plain[17:47]) and torch.equal(got[:16], plain[:16])
    assert not net.module._graph_mode and not net.module._graph_per_stream


def test_run_video_cut_inside_a_chunk(hip, net, edited_clip):
    """A cut at 21 of chunks of 16: the second scene's batches differ from those of its own clip (the chunk grid is the whole clip's), so
    the fields agree to ~1e-6 and the bytes as tests/test_hip_stream.py's sharded clip does: 1 LSB at most, on fewer than 1e-3 of them."""
    from pwstablenet_amd.stream import VideoStabilizer
    src = torch.cat([edited_clip[:21], edited_clip[32:]]).cuda()          # scenes of 21 and 16 frames
    vs = VideoStabilizer(net, batch=8, swap_rb=True)
    got = vs.run_video(src, chunk=16, scene_cuts=[21])
    assert vs.scene_cuts == [21]
    want = torch.cat([vs.run_video(src[:21], chunk=16), vs.run_video(src[21:], chunk=16)])
    d = (got.cpu().numpy().astype(np.int16) - want.cpu().numpy().astype(np.int16))
    d = np.abs(d)
    print("cut inside a chunk: max %d LSB, share of differing bytes %.3g" % (d.max(), float(np.mean(d > 0))))
    assert d.max() <= 1 and np.mean(d > 0) < 1e-3, (d.max(), float(np.mean(d > 0)))
    assert torch.equal(got[:16], want[:16])           # the first chunk holds the first scene's first two batches, as its own clip does


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_run_video_cut_yuv_formats_ride_along(hip, net, fmt):
    """(288 x 320: run_video computes the window planes itself, and INTER_AREA to 256 x 256 refuses a smaller source)"""
    from pwstablenet_amd.stream import VideoStabilizer
    T, h, w = 32, 288, 320
    y = np.concatenate([synth.smooth_frames_u8(1, 16, h, w, 31)[0], synth.smooth_frames_u8(1, 16, h, w, 32)[0]]).astype(np.int64)
    if fmt == "nv12":
        clip = np.concatenate([(16 + y * 219 // 255).astype(np.uint8), np.full((T, h // 2, w), 128, np.uint8)], 1)
    else:
        clip = np.concatenate([((64 + y * 876 // 255) << 6).astype(np.uint16), np.full((T, h // 2, w), 512 << 6, np.uint16)], 1)
    src = torch.from_numpy(clip).cuda()
    vs = VideoStabilizer(net, batch=8)
    got = vs.run_video(src, chunk=8, pixel_format=fmt, scene_cuts=[16])
    want = torch.cat([vs.run_video(src[:16], chunk=8, pixel_format=fmt), vs.run_video(src[16:], chunk=8, pixel_format=fmt)])
    plain = vs.run_video(src, chunk=8, pixel_format=fmt)
    assert got.dtype == src.dtype and got.shape == src.shape
    as_int = (lambda t: t.view(torch.int16)) if fmt == "p010" else (lambda t: t)
    assert torch.equal(as_int(got), as_int(want)) and not torch.equal(as_int(got), as_int(plain))


def _gray_clip(seeds, n=20):
    """frames whose window planes are make_window's: 256 x 256 gray, replicated to three channels"""
    g = np.concatenate([synth.smooth_frames_u8(1, n, 256, 256, s)[0] for s in seeds])
    return torch.from_numpy(np.repeat(g[..., None], 3, -1).copy())


@pytest.mark.parametrize("pair,on_host,in_flight", [(p, k % 2 == 1, 1 + k % 3 // 2) for k, p in enumerate(SEED_PAIRS)])
def test_run_video_finds_the_cut_itself(hip, net, pair, on_host, in_flight):
    from pwstablenet_amd.stream import VideoStabilizer, find_scene_cuts, scene_scores, window_planes
    clip = _gray_clip(pair)
    planes = window_planes(clip.cuda())
    want_planes = np.concatenate([synth.make_window(1, 20, 256, s)[0] for s in pair])
    assert np.abs(planes.cpu().numpy() - want_planes).max() < 1e-6        # the planes are the frames
    scores = scene_scores(planes)
    print("scores: within max %.3f, join %.3f" % (float(torch.cat([scores[:20], scores[21:]]).max()), float(scores[20])))
    assert find_scene_cuts(scores) == [20]
    src = clip.pin_memory() if on_host else clip.cuda()
    vs = VideoStabilizer(net, batch=8)
    got = vs.run_video(src, chunk=16, in_flight=in_flight, scene_cuts="auto")
    assert vs.scene_cuts == [20]
    want = vs.run_video(src, chunk=16, in_flight=in_flight, scene_cuts=[20])
    assert vs.scene_cuts == [20] and torch.equal(got, want)
    assert not torch.equal(got, vs.run_video(src, chunk=16, in_flight=in_flight))
    # thresholds travel: nothing is a cut above the join's score, and a long minimum scene length refuses it too
    vs.run_video(src, chunk=16, scene_cuts="auto", scene_threshold=0.9)
    assert vs.scene_cuts == []
    vs.run_video(src, chunk=16, scene_cuts="auto", scene_min_len=21)
    assert vs.scene_cuts == []


def test_run_video_auto_on_one_scene_changes_nothing(hip, net):
    from pwstablenet_amd.stream import VideoStabilizer
    clip = _gray_clip([14], n=40).pin_memory()
    vs = VideoStabilizer(net, batch=8)
    vs.scene_cuts = [3]
    want = vs.run_video(clip, chunk=16, in_flight=2)
    assert vs.scene_cuts == []
    got = vs.run_video(clip, chunk=16, in_flight=2, scene_cuts="auto")
    assert vs.scene_cuts == [] and torch.equal(got, want)
    # a shard with halos may detect too (its list is in the shard's index space)
    shard = vs.run_video(clip, chunk=16, halo_left=5, halo_right=7, scene_cuts="auto")
    assert vs.scene_cuts == [] and torch.equal(shard, vs.run_video(clip, chunk=16, halo_left=5, halo_right=7))


@pytest.mark.parametrize("on_host,in_flight,detect", [(False, 1, False), (True, 2, True)])
def test_run_video_auto_crop_across_a_cut(hip, net, on_host, in_flight, detect):
    """crop="auto" with a cut == the window of the per-scene recurrence given by hand, with the bounds of the per-scene fields (chunk = the
    scene length: pass 1 forms each scene's batches exactly as _fields does for the scene's own clip)."""
    from pwstablenet_amd.stream import VideoStabilizer, auto_crop_window, field_homography, window_planes
    c, H, W = 34, 360, 640
    frames = torch.from_numpy(np.concatenate([_clip_u8(c, H, W, 17), _clip_u8(c, H, W, 23)]))
    vs = VideoStabilizer(net, batch=8, swap_rb=True)
    planes = window_planes(frames.cuda())
    fields = torch.empty((2 * c, 256, 256, 2), device="cuda")
    with torch.no_grad():
        vs._fields(planes[:c], 0, 0, fields[:c])
        vs._fields(planes[c:], 0, 0, fields[c:])
    _, bounds = field_homography(fields, (H, W))
    window = auto_crop_window(bounds, (H, W), (H // 2, W // 2), vs.period, scene_cuts=[c])
    x0, x1, y0, y1 = window
    assert torch.isfinite(bounds).all() and 0 <= x0 < x1 <= W // 2 and 0 <= y0 < y1 <= H // 2, window
    src = frames.pin_memory() if on_host else frames.cuda()
    want = vs.run_video(src, chunk=c, half_size_output=True, crop=window, in_flight=in_flight, scene_cuts=[c])
    got = vs.run_video(src, chunk=c, half_size_output=True, crop="auto", in_flight=in_flight, scene_cuts="auto" if detect else [c])
    assert vs.scene_cuts == [c]
    assert got.shape == want.shape == (2 * c, int(y1) - int(y0), int(x1) - int(x0), 3) and torch.equal(got, want)


def test_run_video_scene_cut_errors(hip, net, edited_clip):
    from pwstablenet_amd.stream import VideoStabilizer
    vs = VideoStabilizer(net, batch=8)
    src = edited_clip[:20].cuda()
    for bad in ([12, 5], [5, 5], [0], [20], [25], "detect", "Auto"):
        with pytest.raises(ValueError):
            vs.run_video(src, chunk=16, scene_cuts=bad)
    with pytest.raises(ValueError):
        vs.run_video(src, chunk=16, halo_left=2, halo_right=2, scene_cuts=[20])      # indices are in frames' space: 1 .. 19
    out = vs.run_video(src, chunk=16, halo_left=2, halo_right=2, scene_cuts=[1, 19])   # both inside the halos
    assert out.shape[0] == 16
