"""GPU tests of deblurring in the streaming stabiliser, VideoStabilizer(deblur=R): deblur=0 is the stabiliser without the argument bit for
bit; with deblur=2 the frames are those assembled by hand from the same steps -- kept fields, frame_sharpness, global_motion of the input
planes in frame pixels, deblur_plan, the clip deblurred in ONE deblur_frames call, the format's fused warp -- bit for bit; every ValueError;
and on a clip with blurred frames the output frame's sharpness rises by the factor that tests/deblur_ref.py predicts.
A stub generator (a fixed zoomed-out field plus a wave that depends on the window), clips of 20 frames, chunk 8, a cut at 11, in_flight 1
and 2.  The frames are 320 x 256, not smaller: run_video's window planes only scale down, so 256 x 256 is the least it takes; the
crop="auto" case runs at 640 x 320, which holds the homography fit's lattice."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deblur_ref as D  # noqa: E402

T, H, W, CHUNK, CUT, R = 20, 256, 320, 8, 11, 2
BLURRED = (5, 14)
ATTRS = ("deblur_sharpness", "deblur_donors")


class _FieldStub:
    """A generator stand-in: every window's field is ``scale`` times the identity grid plus ``wave`` times the window's centre sample, so
    fields differ from frame to frame and do not depend on how the windows are batched."""
    _graph_mode = _graph_alias = _graph_per_stream = False
    two_queues = None

    def __init__(self, scale=1.03, wave=0.01, align_corners=False):
        self.scale, self.wave, self.align_corners = scale, wave, align_corners

    def enable_graph(self, *args, **kwargs):
        pass

    def __call__(self, x, is_training):
        assert is_training is False
        lin = torch.linspace(-1.0, 1.0, 256, device=x.device)
        yy, xx = torch.meshgrid(lin, lin, indexing="ij")
        grid = torch.stack([xx, yy], -1).unsqueeze(0) * self.scale
        return (grid + self.wave * x[:, x.shape[1] // 2, 128, 128].reshape(-1, 1, 1, 1)).contiguous()


class _Stub:
    def __call__(self, x, is_training):
        raise AssertionError("the generator must not run")


def _gray(h, w):
    """Two scenes of a translating texture with one blurred frame each."""
    a, _ = D.texture(CUT, h, w, 31, blurred=(BLURRED[0],), lam=(5.0, 40.0))
    b, _ = D.texture(T - CUT, h, w, 32, velocity=(-0.75, 1.0), blurred=(BLURRED[1] - CUT,), lam=(5.0, 40.0))
    return np.concatenate([a, b])


@pytest.fixture(scope="module")
def clips():
    g = _gray(H, W)
    return {fmt: torch.from_numpy(D.to_format(g, fmt, 3)).cuda() for fmt in ("bgr24", "nv12", "p010")}


def _planes(src, fmt):
    from pwstablenet_amd import stream as S
    return S.window_planes(src) if fmt == "bgr24" else S.window_planes_yuv(src, fmt) if src.dtype == torch.uint8 else S.window_planes_yuv16(src, fmt)


def _by_hand(vs, src, fmt, cuts, crop=None):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    h, w = PF.frame_format(fmt, src, "test").frame_shape(src)[1:]
    planes = _planes(src, fmt)
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    half = vs.period // 2
    for cs in range(0, T, CHUNK):   # pass 1's generator calls: per chunk, batches restarting at a cut
        ce = min(T, cs + CHUNK)
        hl, hr = min(half, cs), min(half, T - ce)
        sc = [t - (cs - hl) for t in (cuts or []) if cs - hl < t < ce + hr] or None
        vs._fields(planes[cs - hl:ce + hr], hl, hr, fields[cs:ce], sc)
    kw = dict(align_corners=vs.align_corners, mode=vs.interpolation)
    scale = (w / 256.0, h / 256.0)
    if vs.smooth > 0:
        seen = PF.grid_sample(planes.unsqueeze(1), fields, align_corners=vs.align_corners).squeeze(1)
        d, _ = S.smooth_path(S.global_motion(seen, pixel_scale=scale)[0], vs.smooth, scene_cuts=cuts)
        fields = PF.compose_fields(fields, d, (h, w), **kw)
    sharp = S.frame_sharpness(src, fmt)
    maps, gain, donors = S.deblur_plan(S.global_motion(planes, pixel_scale=scale)[0], sharp, vs.deblur, scene_cuts=cuts)
    deb = PF.deblur_frames(src, maps, gain, pixel_format=fmt, sensitivity=vs.deblur_sensitivity)   # the clip in one call
    out = PF.warp(deb, fields, PF.frame_format(fmt, src, "test"), swap_rb=vs.swap_rb, **kw)
    if vs.edge != "pad":
        PF.edge_borders_(out, deb, fields, vs.edge, fmt, swap_rb=vs.swap_rb, **kw)
    if crop == "auto":
        c = S.auto_crop_window(S.field_homography(fields, (h, w))[1], (h, w), (h, w), vs.period, scene_cuts=cuts)
        out = out[:, int(c[2]):int(c[3]), int(c[0]):int(c[1])]   # (scenes of 11 and 9 frames: the recurrence has no frame to update from)
    return out, deb, {"deblur_sharpness": sharp, "deblur_donors": donors}


def test_deblur_zero_is_the_stabiliser_without_the_argument(hip, clips):
    from pwstablenet_amd.stream import VideoStabilizer
    src = clips["bgr24"]
    plain, zero = VideoStabilizer(_FieldStub(), batch=8), VideoStabilizer(_FieldStub(), batch=8, deblur=0)
    for kw in ({}, {"in_flight": 2, "scene_cuts": [CUT]}):
        assert torch.equal(zero.run_video(src, chunk=CHUNK, **kw), plain.run_video(src, chunk=CHUNK, **kw))
        assert all(getattr(zero, a) is None for a in ATTRS) and all(getattr(plain, a) is None for a in ATTRS)
    vs = VideoStabilizer(_FieldStub(), batch=8, deblur=R)   # a call that deblurred leaves nothing behind for one that does not
    deb = vs.run_video(src, chunk=CHUNK)
    assert all(getattr(vs, a) is not None for a in ATTRS) and not torch.equal(deb, plain.run_video(src, chunk=CHUNK))
    vs.deblur = 0
    assert torch.equal(vs.run_video(src, chunk=CHUNK), plain.run_video(src, chunk=CHUNK)) and all(getattr(vs, a) is None for a in ATTRS)


CASES = [("bgr24", 1, {}, {}), ("bgr24", 2, {}, {}), ("nv12", 1, {}, {}), ("nv12", 2, {}, {}), ("p010", 1, {}, {}), ("p010", 2, {}, {}),
         ("bgr24", 1, {"smooth": 2.0}, {}), ("bgr24", 2, {"edge": "mirror"}, {}), ("bgr24", 1, {}, {"crop": "auto"})]
IDS = ["%s-%d-%s" % (f, n, "-".join("%s" % v for v in list(c.values()) + list(k.values())) or "plain") for f, n, c, k in CASES]


@pytest.mark.parametrize("fmt,in_flight,ctor,call", CASES, ids=IDS)
def test_frames_are_the_by_hand_assembly(hip, clips, fmt, in_flight, ctor, call):
    from pwstablenet_amd.stream import VideoStabilizer
    if call.get("crop") == "auto":   # a size that holds the fit's lattice
        src = torch.from_numpy(D.to_format(_gray(320, 640), fmt, 3)).cuda()
    else:
        src = clips[fmt]
    vs = VideoStabilizer(_FieldStub(), batch=8, deblur=R, swap_rb=True, metrics=(fmt == "nv12"), **ctor)
    got = vs.run_video(src, chunk=CHUNK, in_flight=in_flight, pixel_format=fmt, scene_cuts=[CUT], **call)
    want, deb, pieces = _by_hand(vs, src, fmt, [CUT], call.get("crop"))
    for name, value in pieces.items():
        got_v = getattr(vs, name)
        assert got_v.is_cuda and got_v.dtype == value.dtype and torch.equal(got_v, value), name
    donors = vs.deblur_donors.cpu().numpy()
    assert donors[list(BLURRED)].min() >= 2 and not torch.equal(deb, src)   # the blurred frames found donors: a real blend
    assert got.shape == want.shape and torch.equal(got, want)
    if in_flight == 1 and not ctor and not call:   # host input: the overlap goes up again, the same frames
        again = VideoStabilizer(_FieldStub(), batch=8, deblur=R, swap_rb=True)
        assert torch.equal(again.run_video(src.cpu().pin_memory(), chunk=CHUNK, pixel_format=fmt, scene_cuts=[CUT]).cuda(), want)


def test_deblur_errors(hip):
    from pwstablenet_amd.stream import VideoStabilizer
    for bad in (-1, 16, 2.5, None):
        with pytest.raises(ValueError, match="radius"):
            VideoStabilizer(_Stub(), deblur=bad)
    for bad in (0.0, -4.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sensitivity"):
            VideoStabilizer(_Stub(), deblur=2, deblur_sensitivity=bad)
    frames = torch.zeros((T, H, W, 3), dtype=torch.uint8, device="cuda")
    vs = VideoStabilizer(_Stub(), batch=8, deblur=R)
    with pytest.raises(ValueError, match="whole clip"):
        vs.run_video(frames, halo_left=2)
    with pytest.raises(ValueError, match="whole clip"):
        vs.run_video(frames, halo_right=3)
    for borders in ("keep", "mosaic"):
        with pytest.raises(ValueError, match=borders):
            VideoStabilizer(_Stub(), batch=8, deblur=R, borders=borders).run_video(frames)
    with pytest.raises(ValueError, match="integer pixel formats"):
        vs.run_video(frames.float())
    vs.deblur = 16
    with pytest.raises(ValueError, match="radius"):
        vs.run_video(frames)
    vs.deblur, vs.deblur_sensitivity = R, 0.0
    with pytest.raises(ValueError, match="sensitivity"):
        vs.run_video(frames)
    assert vs.deblur_sharpness is None and vs.deblur_donors is None


def test_the_blurred_frames_come_out_sharper(hip, clips):
    """An identity generator under align_corners=True: the warp returns its source up to the truncation of positions that land a hair
    beside a pixel (a fraction of a percent of S), so the output's sharpness is the deblurred source's.  The restatement predicts the rise
    from the same maps and gains: within 1 %."""
    from pwstablenet_amd import stream as S
    src = clips["nv12"]
    vs = S.VideoStabilizer(_FieldStub(1.0, 0.0, align_corners=True), batch=8, deblur=R)
    out = vs.run_video(src, chunk=CHUNK, pixel_format="nv12", scene_cuts=[CUT])
    s_in, s_out = vs.deblur_sharpness.cpu().numpy(), S.frame_sharpness(out, "nv12").cpu().numpy()
    maps, gain, _ = S.deblur_plan(S.global_motion(_planes(src, "nv12"), pixel_scale=(W / 256.0, H / 256.0))[0], vs.deblur_sharpness, R, scene_cuts=[CUT])
    f = src.cpu().numpy()
    val, has = D.blend(f, maps.cpu().numpy(), gain.cpu().numpy(), 0, None, "nv12", vs.deblur_sensitivity)
    s_ref = D.sharpness(D.assemble(f, val, has, 0, "nv12"), "nv12")
    assert np.array_equal(s_in, D.sharpness(f, "nv12"))
    for t in BLURRED:
        rise, want = s_out[t] / s_in[t], s_ref[t] / s_in[t]
        print("frame %d: S %d -> %d, rise %.4f, the restatement %.4f" % (t, s_in[t], s_out[t], rise, want))
        assert want > 1.02 and abs(rise / want - 1.0) <= 0.01   # (a predicted rise above 2 %: a frame left as it was misses the 1 % clearly)
