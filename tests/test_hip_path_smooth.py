"""GPU tests of the path kernel (csrc/path_smooth.hip; stream.smooth_path, C: pws_path_smooth) against the float64 restatement
tests/path_ref.py.

Scenes of n = 1, 2, 5 and 48 frames under sigma = 0.5 (Re = 2), 4 (Re = 12) and 64 (Re = n - 1: the whole scene, both reflections in every
sum), each with one NaN row where the scene has a row to spare.  Tolerance: 1e-12 on D's linear part and 1e-9 on its translation.  Kernel and
restatement run the same float64 operations in the same order; they differ in the device's exp, log, hypot, atan2, sin and cos, an ulp or
two each.  48 sequential steps accumulate a few ulps each on magnitudes of at most 1e3 pixels -- about 1e-10 pixel -- and the linear part
is of magnitude 1.  The translation's gate leaves a decade and sits six below the resolution of a float32 field."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import path_ref as P  # noqa: E402

SIZES = [1, 2, 5, 48]
SIGMAS = [0.5, 4.0, 64.0]
LINEAR, TRANSLATION = [0, 1, 3, 4], [2, 5]


@functools.lru_cache(maxsize=None)
def _motion(n):
    """A frame-pixel motion as a shaky 1280 x 720 clip gives it: a pan of (12, -5) pixels a frame, jitter of 8 pixels, 0.3 degree and 0.2 %
    of scale; one NaN row in the scenes of 5 and 48 frames."""
    rs = np.random.RandomState(100 + n)
    th = np.deg2rad(0.05 + 0.3 * rs.normal(size=n))
    s = 1.0 + 0.002 * rs.normal(size=n)
    m = np.stack([s * np.cos(th), s * np.sin(th), 12.0 + 8.0 * rs.normal(size=n), -5.0 + 8.0 * rs.normal(size=n)], 1)
    m[0] = (1.0, 0.0, 0.0, 0.0)
    if n >= 5:
        m[n // 2] = (np.nan, 0.0, 1.0, np.inf)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _want(n, sigma):
    return P.path_smooth(_motion(n), sigma)


def _bits(t):
    return t.view(torch.int64)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("n", SIZES)
def test_path_and_corrections_against_float64(hip, n, sigma):
    from pwstablenet_amd.stream import smooth_path
    m = torch.from_numpy(np.array(_motion(n))).cuda()
    d, path = smooth_path(m, sigma)
    assert d.is_cuda and d.dtype == path.dtype == torch.float64 and tuple(d.shape) == (n, 6) and tuple(path.shape) == (n, 4)
    want_path, want_d = _want(n, sigma)
    got_d, got_path = d.cpu().numpy(), path.cpu().numpy()
    e_path = float(np.abs(got_path - want_path).max())
    e_lin = float(np.abs(got_d[:, LINEAR] - want_d[:, LINEAR]).max())
    e_tr = float(np.abs(got_d[:, TRANSLATION] - want_d[:, TRANSLATION]).max())
    print("n %d sigma %g: path %.3g (largest |P| %.3g), D linear %.3g, D translation %.3g (largest %.3g)"
          % (n, sigma, e_path, np.abs(want_path).max(), e_lin, e_tr, np.abs(want_d[:, TRANSLATION]).max()))
    assert e_lin <= 1e-12 and e_tr <= 1e-9 and e_path <= 1e-9
    again = smooth_path(m, sigma)
    assert torch.equal(_bits(again[0]), _bits(d)) and torch.equal(_bits(again[1]), _bits(path))
    if n == 1:
        assert got_d.tolist() == [list(P.IDENTITY)] and got_path.tolist() == [[0.0] * 4]
    if n >= 5:   # the NaN row is the identity row
        clean = np.array(_motion(n))
        clean[n // 2] = (1.0, 0.0, 0.0, 0.0)
        other = smooth_path(torch.from_numpy(clean).cuda(), sigma)
        assert torch.equal(_bits(other[0]), _bits(d)) and torch.equal(_bits(other[1]), _bits(path))


def test_constant_velocity_is_left_alone(hip):
    from pwstablenet_amd.stream import smooth_path
    m = torch.tensor([[1.0, 0.0, 0.8, -0.3]] * 40, dtype=torch.float64, device="cuda")
    d, path = smooth_path(m, 4.0)
    assert float((d - torch.tensor(P.IDENTITY, dtype=torch.float64, device="cuda")).abs().max()) <= 1e-12
    assert float((path[-1] - torch.tensor([0.0, 0.0, 39 * 0.8, 39 * -0.3], dtype=torch.float64, device="cuda")).abs().max()) <= 1e-12


def test_scenes_are_smoothed_apart(hip):
    from pwstablenet_amd.stream import smooth_path
    m = torch.from_numpy(np.array(_motion(48))).cuda()
    d, path = smooth_path(m, 4.0, scene_cuts=[20, 21])   # (a scene of one frame between two others)
    for a, b in ((0, 20), (20, 21), (21, 48)):
        da, pa = smooth_path(m[a:b].contiguous(), 4.0)
        assert torch.equal(_bits(d[a:b].contiguous()), _bits(da)) and torch.equal(_bits(path[a:b].contiguous()), _bits(pa))
    assert d[20].tolist() == list(P.IDENTITY) and not path[20].any() and not path[21].any()
    want = P.smooth_path(_motion(48), 4.0, [20, 21])
    assert np.abs(d.cpu().numpy() - want[0]).max() <= 1e-9
    empty = smooth_path(m[:0], 4.0)
    assert tuple(empty[0].shape) == (0, 6) and tuple(empty[1].shape) == (0, 4)


def test_path_errors(hip):
    from pwstablenet_amd.stream import smooth_path
    m = torch.zeros((5, 4), dtype=torch.float64, device="cuda")
    for bad in (0.0, -1.0, 256.5, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="sigma"):
            smooth_path(m, bad)
    for bad in (m.float(), m.cpu(), m[:, :3], m[0], m.cpu().numpy()):
        with pytest.raises(ValueError, match="motion"):
            smooth_path(bad, 4.0)
    with pytest.raises(ValueError, match="scene_cuts"):
        smooth_path(m, 4.0, scene_cuts=[5])
    L, Pt = hip.lib(), hip.ptr
    path, d = torch.full((5, 4), 7.0, dtype=torch.float64, device="cuda"), torch.full((5, 6), 7.0, dtype=torch.float64, device="cuda")
    for sigma in (0.0, -2.0, 256.0001, float("nan")):
        assert L.pws_path_smooth(Pt(m), 5, sigma, Pt(path), Pt(d), None) == -22 and b"sigma" in L.pws_last_error()
    assert L.pws_path_smooth(None, 5, 4.0, Pt(path), Pt(d), None) == -22 and b"NULL" in L.pws_last_error()
    assert L.pws_path_smooth(Pt(m), 5, 4.0, None, Pt(d), None) == -22 and L.pws_path_smooth(Pt(m), 5, 4.0, Pt(path), None, None) == -22
    assert L.pws_path_smooth(Pt(m), -1, 4.0, Pt(path), Pt(d), None) == -22
    assert L.pws_path_smooth(hip.ctypes.c_void_p(m.data_ptr() + 4), 4, 4.0, Pt(path), Pt(d), None) == -22 and b"aligned" in L.pws_last_error()
    assert L.pws_path_smooth(None, 0, 4.0, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((path == 7.0).all()) and bool((d == 7.0).all())
    assert L.pws_path_smooth(Pt(m), 5, 256.0, Pt(path), Pt(d), None) == 0   # the largest sigma
    torch.cuda.synchronize()
