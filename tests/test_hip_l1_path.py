"""GPU tests of the L1-optimal path (csrc/path_l1.hip; stream.optimal_path, C: pws_l1_path) against linear programs solved by HiGHS
(tests/golden/l1_path.npz) and against the float64 restatement tests/l1_path_ref.py.

Every golden case runs as the x component of a translation-only motion: motion[k] = (1, 0, P[k] - P[k-1], 0).  There the scan is exact
(exp(0) = cos(0) = 1, sin(0) = 0), ``path[:, 2]`` is the running sum of the differences, and D[:, 2] = 1 * (1 * ux + 0 * uy) IS ux = P^ - P as
the kernel formed it, so feasibility can be asked exactly.  The frame and the reach are chosen so that c W / 2 is the case's box bit for
bit: reach 0.125 of W = 16 b, and reach 0.05 of W = 2 for the box of 0.05."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import l1_path_ref as L  # noqa: E402
import path_ref as P  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "l1_path.npz"))
CASES = ("walk4", "walk5", "walk9", "walk200", "walk513", "ramp", "jolt", "constant", "shake", "angle")
# the restatement's largest distance from HiGHS's minimiser where the optimum is unique, in the path's units, measured on the CPU
# (tests/test_l1_path_ref_cpu.py's solves): the kernel may lie 100 x that from the restatement, never more than 1e-3 b
REF_TO_HIGHS = {"ramp": 1.052e-10, "jolt": 1.408e-8, "walk200": 7.894e-7, "walk513": 2.279e-6}
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def _bits(t):
    return t.view(torch.int64)


def _frame(b):
    """(frame_hw, reach) under which optimal_path's box in x is b exactly."""
    hw, reach = ((2, 2), 0.05) if b == 0.05 else ((int(8 * b), int(16 * b)), 0.125)
    assert L.bounds(reach, hw)[2] == b
    return hw, reach


def _translation(p):
    m = np.zeros((len(p), 4), np.float64)
    m[:, 0] = 1.0
    m[1:, 2] = np.diff(p)
    return m


_runs = {}


def _run(name):
    """(motion, b, frame_hw, reach, D, path, info) of a golden case, computed once and left unchanged."""
    if name not in _runs:
        from pwstablenet_amd.stream import optimal_path
        b = float(GOLDEN[name + "_b"])
        hw, reach = _frame(b)
        motion = _translation(GOLDEN[name + "_P"])
        d, path, info = optimal_path(torch.from_numpy(motion).cuda(), hw, reach, return_info=True)
        _runs[name] = (motion, b, hw, reach, d, path, info)
    return _runs[name]


@pytest.mark.parametrize("name", CASES)
def test_against_the_lp_optimum(hip, name):
    """The measured path is smooth_path's bit for bit; |P^ - P| <= b exactly; the objective within 1e-6 f_LP + 1e-6 max(w) b of HiGHS's
    optimum (the reference is HiGHS, not the code under test); every component converged within 64 steps."""
    from pwstablenet_amd.stream import smooth_path
    motion, b, hw, reach, d, path, info = _run(name)
    n = len(motion)
    assert d.is_cuda and d.dtype == path.dtype == info.dtype == torch.float64
    assert tuple(d.shape) == (n, 6) and tuple(path.shape) == (n, 4) and tuple(info.shape) == (1, 4, 4)
    assert torch.equal(_bits(path), _bits(smooth_path(torch.from_numpy(motion).cuda(), 4.0)[1]))
    got_d, got_p, got_i = d.cpu().numpy(), path.cpu().numpy()[:, 2], info.cpu().numpy()[0]
    assert np.array_equal(got_d[:, [0, 1, 3, 4, 5]], np.tile([1.0, 0.0, 0.0, 1.0, 0.0], (n, 1)))   # nothing but x moves
    u = got_d[:, 2]
    assert np.all(np.abs(u) <= b)
    f, f_lp = L.objective(got_p + u), float(GOLDEN[name + "_f"])
    print("%s: n %d steps %s eta %.3g f %.12g f_LP %.12g gap %.3g" % (name, n, got_i[:, 0].tolist(), got_i[2, 1], f, f_lp, f - f_lp))
    assert f - f_lp <= 1e-6 * f_lp + 1e-6 * max(L.WEIGHTS) * b
    assert (got_i[:, 3] == 1.0).all() and (got_i[:, 0] <= 64).all()
    assert got_i[[0, 1, 3]].tolist() == [got_i[0].tolist()] * 3   # the three still components: the same zero path, the same iteration


@pytest.mark.parametrize("name", sorted(REF_TO_HIGHS))
def test_against_the_restatement(hip, name):
    """Where the optimum is unique the kernel's path lies within 100 x the restatement's own distance from HiGHS (measured on the CPU: ramp
    1.052e-10, jolt 1.408e-8, walk200 7.894e-7, walk513 2.279e-6 px), and never further than 1e-3 b: the two run the same operations in
    the same order, and what differs -- nothing but the division and the square root's rounding, if anything -- is amplified by the last
    systems' conditioning."""
    motion, b, hw, reach, d, path, info = _run(name)
    D, Pm, U, ref_info = L.optimal_path(motion, hw, reach)
    assert np.array_equal(path.cpu().numpy(), Pm)   # (a translation's scan is exact on both sides)
    dist = float(np.abs(d.cpu().numpy()[:, 2] - U[:, 2]).max())
    gate = min(100.0 * REF_TO_HIGHS[name], 1e-3 * b)
    print("%s: kernel to restatement %.3g px (gate %.3g); steps %g / %g" % (name, dist, gate, info[0, 2, 0].item(), ref_info[0, 2, 0]))
    assert dist <= gate


def _shaky(n, seed):
    """tests/test_hip_path_smooth.py's frame-pixel motion of a shaky 1280 x 720 clip, with one NaN row."""
    rs = np.random.RandomState(seed)
    th = np.deg2rad(0.05 + 0.3 * rs.normal(size=n))
    s = 1.0 + 0.002 * rs.normal(size=n)
    m = np.stack([s * np.cos(th), s * np.sin(th), 12.0 + 8.0 * rs.normal(size=n), -5.0 + 8.0 * rs.normal(size=n)], 1)
    m[0] = (1.0, 0.0, 0.0, 0.0)
    m[n // 2] = (np.nan, 0.0, 1.0, np.inf)
    return m


def test_all_four_components_runs_nan_rows_and_cuts(hip):
    """A similarity motion, 300 frames (two rounds of the 256 threads): every component against the restatement run on the kernel's own
    measured path (the scan's exp, log, sin, cos and atan2 differ by an ulp or two between device and host; from the same path the solver's
    operations are the same on both sides) -- D's linear part within 1e-9, its translation within 1e-6 px, as above a margin for the last
    systems' conditioning; then: two runs are the same bits, a NaN row is the (1, 0, 0, 0) row, cuts are the per-slice calls."""
    from pwstablenet_amd.stream import optimal_path, smooth_path
    n, hw = 300, (720, 1280)
    m = _shaky(n, 7)
    mt = torch.from_numpy(m).cuda()
    d, path, info = optimal_path(mt, hw, return_info=True)
    assert torch.equal(_bits(path), _bits(smooth_path(mt, 4.0)[1]))
    assert np.abs(path.cpu().numpy() - P.camera_path(m)).max() <= 1e-9
    Pk, b = path.cpu().numpy(), L.bounds(0.1, hw)
    U = np.stack([L.solve_component(Pk[:, c], b[c])[0] for c in range(4)], 1)
    want, got = L.corrections(Pk, U), d.cpu().numpy()
    e_lin, e_tr = float(np.abs(got[:, [0, 1, 3, 4]] - want[:, [0, 1, 3, 4]]).max()), float(np.abs(got[:, [2, 5]] - want[:, [2, 5]]).max())
    print("D linear %.3g, translation %.3g px; steps %s; largest |U| / b %s" % (e_lin, e_tr, info[0, :, 0].tolist(), (np.abs(U).max(0) / b).tolist()))
    assert e_lin <= 1e-9 and e_tr <= 1e-6
    assert bool((info[0, :, 3] == 1.0).all()) and float(np.abs(U).max()) > 1.0   # a real correction
    again = optimal_path(mt, hw, return_info=True)
    assert all(torch.equal(_bits(a), _bits(b_)) for a, b_ in zip(again, (d, path, info)))
    clean = m.copy()
    clean[n // 2] = (1.0, 0.0, 0.0, 0.0)
    other = optimal_path(torch.from_numpy(clean).cuda(), hw, return_info=True)
    assert all(torch.equal(_bits(a), _bits(b_)) for a, b_ in zip(other, (d, path, info)))
    cuts = [40, 41, 43, 200]   # scenes of 40, 1, 2, 157 and 100 frames
    dc, pc, ic = optimal_path(mt, hw, scene_cuts=cuts, return_info=True)
    assert tuple(ic.shape) == (5, 4, 4)
    for i, (a, e) in enumerate(zip([0] + cuts, cuts + [n])):
        ds, ps, is_ = optimal_path(mt[a:e].contiguous(), hw, return_info=True)
        assert torch.equal(_bits(dc[a:e].contiguous()), _bits(ds)) and torch.equal(_bits(pc[a:e].contiguous()), _bits(ps))
        assert torch.equal(_bits(ic[i:i + 1].contiguous()), _bits(is_))
    assert dc[40:43].tolist() == [IDENTITY] * 3 and ic[1:3, :, :].tolist() == [[[0.0, 0.0, 0.0, 1.0]] * 4] * 2


def test_short_scenes_are_the_identity(hip):
    from pwstablenet_amd.stream import optimal_path
    for n in range(4):
        m = torch.tensor([[1.0, 0.0, 3.0, -2.0]] * n, dtype=torch.float64, device="cuda").reshape(n, 4)
        d, path, info = optimal_path(m, (720, 1280), return_info=True)
        assert tuple(d.shape) == (n, 6) and tuple(path.shape) == (n, 4) and tuple(info.shape) == (1 if n else 0, 4, 4)
        assert d.tolist() == [IDENTITY] * n and info.tolist() == ([[[0.0, 0.0, 0.0, 1.0]] * 4] if n else [])
        assert path.tolist() == [[0.0, 0.0, 3.0 * k, -2.0 * k] for k in range(n)]
    assert len(optimal_path(torch.zeros((0, 4), dtype=torch.float64, device="cuda"), (720, 1280))) == 2


def test_errors(hip):
    from pwstablenet_amd.stream import optimal_path
    m = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * 5, dtype=torch.float64, device="cuda")   # a still camera
    hw = (720, 1280)
    for bad in (m.float(), m.cpu(), m[:, :3], m[0], m.cpu().numpy()):
        with pytest.raises(ValueError, match="optimal_path: motion must be a \\(T, 4\\) float64 tensor on the device"):
            optimal_path(bad, hw)
    for bad in (0.0, -0.1, 0.51, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="optimal_path: reach must lie in \\(0, 0.5\\], got"):
            optimal_path(m, hw, reach=bad)
    with pytest.raises(ValueError, match="optimal_path: reach must be a share of the frame in \\(0, 0.5\\], got 'x'"):
        optimal_path(m, hw, reach="x")
    for bad in ((1.0, 2.0), (1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, float("inf"), 1.0), 3.0, ("a", 1, 1)):
        with pytest.raises(ValueError, match="optimal_path: weights must be three positive finite numbers \\(w1, w2, w3\\), got"):
            optimal_path(m, hw, weights=bad)
    with pytest.raises(ValueError, match="scene_cuts"):
        optimal_path(m, hw, scene_cuts=[5])
    for bad in ((720,), 720, ("a", "b"), None):
        with pytest.raises(ValueError, match="optimal_path: frame_hw must be \\(H, W\\), got"):
            optimal_path(m, bad)
    with pytest.raises(ValueError, match="optimal_path: the frame must be at least 2 x 2 pixels, got 1280 x 1"):
        optimal_path(m, (1, 1280))
    with pytest.raises(ValueError, match="optimal_path: a scene of 65537 frames, at most 65536"):
        optimal_path(torch.zeros((65537, 4), dtype=torch.float64, device="cuda"), hw)
    assert optimal_path(m, hw, reach=0.5, weights=[1, 1, 1])[0].tolist() == [IDENTITY] * 5   # the largest reach; no motion, no correction

    L_, Pt, C = hip.lib(), hip.ptr, hip.ctypes
    nbytes = L_.pws_l1_path_workspace(5)
    assert nbytes == 5 * 144 * 8 and L_.pws_l1_path_workspace(0) == 0 and L_.pws_l1_path_workspace(-3) == 0
    path, d = torch.full((5, 4), 7.0, dtype=torch.float64, device="cuda"), torch.full((5, 6), 7.0, dtype=torch.float64, device="cuda")
    info, ws = torch.full((4, 4), 7.0, dtype=torch.float64, device="cuda"), torch.empty((nbytes // 8,), dtype=torch.float64, device="cuda")
    bound, wts = (C.c_double * 4)(0.1, 0.05, 64.0, 36.0), (C.c_double * 3)(10.0, 1.0, 100.0)

    def call(motion=Pt(m), n=5, b=bound, w=wts, p=Pt(path), dd=Pt(d), i=Pt(info), wsp=Pt(ws), nb=nbytes):
        return L_.pws_l1_path(motion, n, b, w, p, dd, i, wsp, nb, None)
    for k in range(4):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            bad = (C.c_double * 4)(*[v if j == k else 1.0 for j in range(4)])
            assert call(b=bad) == -22 and b"bound[%d]" % k in L_.pws_last_error()
    for k in range(3):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            bad = (C.c_double * 3)(*[v if j == k else 1.0 for j in range(3)])
            assert call(w=bad) == -22 and b"weights[%d]" % k in L_.pws_last_error()
    assert call(b=None) == -22 and b"NULL" in L_.pws_last_error() and call(w=None) == -22
    for kw in ({"motion": None}, {"p": None}, {"dd": None}, {"i": None}, {"wsp": None}):
        assert call(**kw) == -22 and b"NULL" in L_.pws_last_error()
    assert call(n=-1) == -22 and b"bad shape" in L_.pws_last_error()
    assert call(n=65537) == -22 and b"at most 65536" in L_.pws_last_error()
    assert call(nb=nbytes - 8) == -22 and b"workspace" in L_.pws_last_error()
    assert call(motion=C.c_void_p(m.data_ptr() + 4), n=4) == -22 and b"aligned" in L_.pws_last_error()
    assert call(wsp=C.c_void_p(ws.data_ptr() + 4), nb=nbytes - 8, n=4) == -22 and b"aligned" in L_.pws_last_error()
    assert L_.pws_l1_path(None, 0, bound, wts, None, None, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((path == 7.0).all()) and bool((d == 7.0).all()) and bool((info == 7.0).all())   # no failed call launched anything
    assert call() == 0
    torch.cuda.synchronize()
    assert d.tolist() == [IDENTITY] * 5 and bool((info[:, 3] == 1.0).all())
