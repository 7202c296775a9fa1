"""GPU tests of the automatic crop (reference main_new.py:484-606): pws_field_homography against the float64 restatement in
tests/homography_ref.py, and VideoStabilizer.run_video(crop="auto") against run_video with the same window given by hand."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_ref as R  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402


def _base(n=256):
    u = torch.linspace(-1, 1, n, dtype=torch.float64)
    yy, xx = torch.meshgrid(u, u, indexing="ij")
    return xx, yy


def _field(P, eps=0.0, phase=0.0):
    """(256, 256, 2): pixel p of the output samples the source at pi(P [p, 1]) + eps * a smooth residual."""
    xx, yy = _base()
    w = P[2][0] * xx + P[2][1] * yy + P[2][2]
    fx = (P[0][0] * xx + P[0][1] * yy + P[0][2]) / w + eps * torch.sin(np.pi * xx + phase) * torch.cos(0.5 * np.pi * yy)
    fy = (P[1][0] * xx + P[1][1] * yy + P[1][2]) / w + eps * torch.cos(np.pi * yy - phase) * torch.sin(0.7 * np.pi * xx)
    return torch.stack([fx, fy], -1).float()


FAMILY = [
    ([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], 0.0),
    ([[1.08, 0.03, 0.02], [-0.02, 1.06, -0.01], [0.0, 0.0, 1.0]], 0.0),
    ([[1.05, 0.02, -0.03], [0.01, 1.1, 0.02], [0.03, -0.02, 1.0]], 0.0),
    ([[1.05, 0.02, -0.03], [0.01, 1.1, 0.02], [0.03, -0.02, 1.0]], 0.01),
    ([[0.95, -0.04, 0.01], [0.05, 1.02, -0.02], [-0.04, 0.025, 1.0]], 0.02),
    ([[1.12, 0.0, 0.05], [0.0, 1.12, -0.04], [0.01, 0.01, 1.0]], 0.005),
]


@pytest.mark.parametrize("frame_hw", [(360, 640), (720, 1280)])
def test_samples_are_the_live_resize_bit_for_bit(hip, frame_hw):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.stream import field_homography
    g = torch.Generator().manual_seed(3)
    field = (torch.rand((3, 256, 256, 2), generator=g) * 2 - 1).cuda()
    _, _, pts = field_homography(field, frame_hw, return_points=True)
    up = PF.upsample_bilinear2d(field.permute(0, 3, 1, 2).contiguous(), frame_hw).permute(0, 2, 3, 1)
    r, c, _ = R.lattice(frame_hw)
    want = up[:, torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda(), :]
    assert pts.shape == (3, 400, 2) and torch.equal(pts, want)


@pytest.mark.parametrize("frame_hw", [(360, 640), (720, 1280)])
def test_fit_and_bounds_match_the_float64_restatement(hip, frame_hw):
    from pwstablenet_amd.stream import field_homography
    field = torch.stack([_field(P, eps, phase=k) for k, (P, eps) in enumerate(FAMILY)]).cuda()
    M, bounds, pts = field_homography(field, frame_hw, return_points=True)
    M, bounds, pts = M.cpu().numpy(), bounds.cpu().numpy(), pts.cpu().numpy().astype(np.float64)
    _, _, p2 = R.lattice(frame_hw)
    h0, w0 = frame_hw
    for k in range(len(FAMILY)):
        ref = R.fit(pts[k], p2)
        assert ref is not None and np.all(np.isfinite(M[k]))
        assert M[k].reshape(3, 3)[2, 2] == 1.0
        assert np.abs(R.corners(M[k].reshape(3, 3)) - R.corners(ref)).max() < 1e-6, k
        tol = np.array([h0, h0, w0, w0]) / 2 * 1e-6 + 2.5e-4            # 1e-6 normalised + the fp32 rounding of a pixel position
        assert np.all(np.abs(bounds[k] - R.bounds(ref, frame_hw)) < tol), (k, bounds[k], R.bounds(ref, frame_hw))
    # an affine field is recovered exactly: M is the inverse of the map from a lattice pixel's position p2 (= 2 r / H0 - 1) to the
    # field's sample there, P u with u = 2 r / (H0 - 1) - 1 (the resize's align_corners grid)
    sx, sy = w0 / (w0 - 1), h0 / (h0 - 1)
    U = np.array([[sx, 0, sx - 1], [0, sy, sy - 1], [0, 0, 1.0]])
    want = np.linalg.inv(np.array(FAMILY[1][0]) @ U)
    assert np.abs(M[1].reshape(3, 3) - want / want[2, 2]).max() < 1e-5


def test_constant_field_gives_nan_not_garbage(hip):
    from pwstablenet_amd.stream import field_homography
    field = torch.full((2, 256, 256, 2), 0.3, device="cuda")
    field[1] = _field(FAMILY[2][0]).cuda()
    M, bounds = field_homography(field, (360, 640))
    assert torch.isnan(M[0]).all() and torch.isnan(bounds[0]).all()
    assert torch.isfinite(M[1]).all() and torch.isfinite(bounds[1]).all()   # its neighbour in the launch is unaffected
    with pytest.raises(ValueError):
        field_homography(field, (299, 640))
    with pytest.raises(ValueError):
        field_homography(field, (360, 599))


def _net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    net = define_G(31, 2, 16, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=16)})
    return net.cuda()


def _clip(T, H, W, seed):
    rs = np.random.RandomState(seed)
    base = synth.smooth_frames_u8(1, T, H, W, seed)[0]
    col = np.stack([base * 0.9, base * 1.0, base * 0.8], -1) + rs.randint(-3, 4, (T, H, W, 3))
    return torch.from_numpy(np.clip(col, 0, 255).astype(np.uint8))


@pytest.mark.parametrize("on_host,in_flight,out_mode,graph", [(True, 1, "half", False), (False, 2, "size", False),
                                                              (True, 2, "half", True), (False, 1, None, True), (True, 1, None, False)])
def test_run_video_auto_equals_the_window_given_by_hand(hip, on_host, in_flight, out_mode, graph):
    from pwstablenet_amd.stream import VideoStabilizer, auto_crop_window, field_homography, window_planes
    net = _net()
    T, H, W = 36, 360, 640
    frames = _clip(T, H, W, 17)
    vs = VideoStabilizer(net, batch=8, swap_rb=True)
    # the bounds as pass 1 computes them: the same windows per generator call (chunks of 16 = two batches of 8)
    planes = window_planes(frames.cuda())
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    with torch.no_grad():
        vs._fields(planes, 0, 0, fields)
    _, bounds = field_homography(fields, (H, W))
    kw = {"half": {"half_size_output": True}, "size": {"output_size": (480, 270)}, None: {}}[out_mode]
    oh, ow = {"half": (H // 2, W // 2), "size": (270, 480), None: (H, W)}[out_mode]
    window = auto_crop_window(bounds, (H, W), (oh, ow), vs.period)
    # the random-weight generator is no stabiliser, but its fields on this clip give finite bounds and a valid window
    x0, x1, y0, y1 = window
    assert torch.isfinite(bounds).all() and 0 <= x0 < x1 <= ow and 0 <= y0 < y1 <= oh, window
    src = frames.pin_memory() if on_host else frames.cuda()
    net.module.enable_graph(graph)
    try:
        want = vs.run_video(src, chunk=16, crop=window, **kw)
        got = vs.run_video(src, chunk=16, crop="auto", in_flight=in_flight, **kw)
        torch.cuda.synchronize()
        assert got.is_cuda != on_host and got.shape == want.shape == (T, int(y1) - int(y0), int(x1) - int(x0), 3)
        assert torch.equal(got, want)
        assert net.module._graph_mode == graph and not net.module._graph_per_stream
    finally:
        net.module.enable_graph(False)


class _AffineStub:
    """A generator stand-in: every window's field is the affine map p -> s p + t; counts the windows it is called on."""

    def __init__(self, s, t):
        self.s, self.t, self.windows, self.calls = s, t, 0, 0

    def __call__(self, x, is_training):
        assert is_training is False
        n = x.shape[0]
        self.windows += n
        self.calls += 1
        xx, yy = _base()
        f = torch.stack([self.s * xx + self.t[0], self.s * yy + self.t[1]], -1).float().cuda()
        return f.unsqueeze(0).expand(n, -1, -1, -1).contiguous()


def _stub_bounds(s, t, frame_hw):
    h0, w0 = frame_hw
    M = np.array([[1 / s, 0, -t[0] / s], [0, 1 / s, -t[1] / s], [0, 0, 1.0]])
    return R.bounds(M, frame_hw)


@pytest.mark.parametrize("on_host", [True, False])
def test_run_video_auto_runs_the_generator_once_per_frame(hip, on_host):
    from pwstablenet_amd.stream import VideoStabilizer
    T, H, W = 37, 360, 640
    s, t = 1.1, (0.04, -0.03)        # zoomed out: the source frame covers less than the output, black wedges on every side
    stub = _AffineStub(s, t)
    vs = VideoStabilizer(stub, batch=8)
    frames = _clip(T, H, W, 5)
    src = frames.pin_memory() if on_host else frames.cuda()
    got = vs.run_video(src, chunk=12, crop="auto", half_size_output=True)
    assert stub.windows == T and stub.calls == 7       # chunks 12, 12, 12, 1 -> batches 8 + 4 per full chunk, 1 for the last
    b = _stub_bounds(s, t, (H, W))
    x0, x1, y0, y1 = R.crop_window(np.tile(b, (T, 1)), (H, W))   # 6 updated frames (16 .. 21)
    x0, x1, y0, y1 = x0 / 2, x1 / 2, y0 / 2, y1 / 2
    # left = ((-1 - 0.04) / 1.1 + 1) * 320 = 17.45 source pixels, ...: (8.59, 298.81, 10.47, 173.72) in the 320 x 180 output
    assert 8 < x0 < 9 and 298 < x1 < 299 and 10 < y0 < 11 and 173 < y1 < 174, (x0, x1, y0, y1)
    for v in (x0, x1, y0, y1):
        assert 0.05 < v - int(v) < 0.95
    assert tuple(got.shape) == (T, int(y1) - int(y0), int(x1) - int(x0), 3)
    stub.windows = stub.calls = 0
    want = vs.run_video(src, chunk=12, crop=(x0, x1, y0, y1), half_size_output=True)
    assert torch.equal(got.cpu(), want.cpu())


def test_run_video_auto_errors(hip):
    from pwstablenet_amd.stream import VideoStabilizer
    T, H, W = 34, 360, 640
    frames = _clip(T, H, W, 9).cuda()
    vs = VideoStabilizer(_AffineStub(1.1, (0.0, 0.0)), batch=8)
    with pytest.raises(ValueError, match="whole clip"):
        vs.run_video(frames, crop="auto", halo_left=2)
    with pytest.raises(ValueError, match="whole clip"):
        vs.run_video(frames, crop="auto", halo_right=1)
    with pytest.raises(ValueError, match="600 x 300"):
        vs.run_video(frames[:, :296, :600].contiguous(), crop="auto")
    with pytest.raises(ValueError):
        vs.run_video(frames, crop="automatic")
    vs = VideoStabilizer(_AffineStub(0.0, (0.2, -0.1)), batch=8)     # a constant field: no homography in any frame
    with pytest.raises(ValueError, match="frame 16"):
        vs.run_video(frames, crop="auto")
    vs = VideoStabilizer(_AffineStub(-1.0, (0.0, 0.0)), batch=8)     # a mirrored frame: left > right, the window closes in 2 updates
    with pytest.raises(ValueError, match="empty"):
        vs.run_video(frames, crop="auto")
