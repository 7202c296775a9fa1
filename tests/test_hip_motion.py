"""GPU tests of the global-motion kernels (csrc/motion.hip) against the numpy restatement (tests/motion_ref.py): pws_block_motion bit for bit,
pws_motion_fit within a tolerance measured from the restatement's own summation orders, repeatability, and the errors."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_ref as R  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402

# (2, 48, 48) R 16: a single block; (3, 64, 80) R 8; (2, 70, 90) R 8: remainder strips, rows that are no multiple of 4 floats; (2, 40, 56) R 4;
# (5, 256, 256) R 16: the live shape, 196 blocks, 1089 candidates (more than four per lane)
SHAPES = [(2, 48, 48, 16), (3, 64, 80, 8), (2, 70, 90, 8), (2, 40, 56, 4), (5, 256, 256, 16)]


def _shifts(radius):
    """whole-pixel shifts inside the range, on its rim and beyond it"""
    m = radius - 1
    return [(0, 0), (m, -m), (-m, m), (radius, 0), (0, -radius), (radius + 3, 2), (-radius - 1, -radius - 1), (1, -2)]


@functools.lru_cache(maxsize=None)
def _inputs(n, h, w, radius):
    rs = np.random.RandomState(n * 100 + h + w)
    uniform = rs.uniform(-1.2, 1.2, (n, h, w)).astype(np.float32)
    flat_idx = rs.choice(uniform.size, 24, replace=False)
    uniform.reshape(-1)[flat_idx] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), 24)
    smooth = synth.smooth_frames_u8(1, n, h, w, seed=h + w)[0]
    out = {"uniform": uniform,
           "window": (smooth.astype(np.float32) / np.float32(255) * np.float32(2) - np.float32(1)).astype(np.float32),
           "rolled": R.rolled_noise(_shifts(radius)[:max(n, 4) if h == 256 else None], h, w, seed=h * w),
           "flat": np.full((n, h, w), -0.3, np.float32)}
    return {k: (v, R.block_motion(v, radius)) for k, v in out.items()}


@pytest.mark.parametrize("shape", SHAPES)
def test_blocks_equal_the_restatement_bit_for_bit(hip, shape):
    from pwstablenet_amd.stream import block_motion
    n, h, w, radius = shape
    nby, nbx = R.lattice(h, w, radius)
    for name, (planes, want) in _inputs(*shape).items():
        d = torch.from_numpy(planes).cuda()
        mv, sad, act = block_motion(d, radius)
        t = planes.shape[0]
        assert (mv.dtype, sad.dtype, act.dtype) == (torch.int16, torch.int32, torch.int32) and mv.is_cuda
        assert mv.shape == (t, nby, nbx, 2) and sad.shape == (t, nby, nbx, 5) and act.shape == (t, nby, nbx)
        for got, ref, what in zip((mv, sad, act), want, ("mv", "sad", "activity")):
            assert np.array_equal(got.cpu().numpy(), ref), (name, what)
        assert not mv[0].any() and not sad[0].any()
        again = block_motion(d, radius)
        assert all(torch.equal(a, b) for a, b in zip(again, (mv, sad, act))), name
        if name == "flat":
            assert not mv.any() and not act.any()
        if name == "rolled":   # the planted shifts inside the range come back with S = 0
            for k, sh in enumerate(_shifts(radius)[:t]):
                if k and max(abs(sh[0]), abs(sh[1])) < radius:
                    assert (mv[k].cpu().numpy() == np.array(sh, np.int16)).all() and not sad[k, ..., 0].any()


def test_one_plane_and_no_plane(hip):
    from pwstablenet_amd.stream import block_motion, global_motion
    planes = _inputs(3, 64, 80, 8)["uniform"][0]
    mv, sad, act = block_motion(torch.from_numpy(planes[:1].copy()).cuda(), 8)
    assert not mv.any() and not sad.any() and np.array_equal(act.cpu().numpy(), R.block_motion(planes[:1], 8)[2])
    motion, inl = global_motion(torch.from_numpy(planes[:1].copy()).cuda(), 8)
    assert motion.cpu().tolist() == [[1.0, 0.0, 0.0, 0.0]] and inl.cpu().tolist() == [0]
    empty = torch.zeros((0, 64, 80), device="cuda")
    assert [tuple(x.shape) for x in block_motion(empty, 8)] == [(0, 3, 4, 2), (0, 3, 4, 5), (0, 3, 4)]
    motion, inl = global_motion(empty, 8)
    assert motion.shape == (0, 4) and motion.dtype == torch.float64 and inl.shape == (0,) and inl.dtype == torch.int32


@functools.lru_cache(maxsize=None)
def _fit_clips():
    """(name, planes, radius, min_activity): the jittered and the steady analytic texture, planted whole-pixel shifts (inside, on and beyond
    the rim), and smooth frames, whose blocks lie on both sides of an
    activity threshold of 1000"""
    jit = R.texture_clip(R.planted_path(6, seed=11, jitter=True), 256, 256, seed=3)
    steady = R.texture_clip(R.planted_path(5, seed=11, jitter=False), 128, 160, seed=4)
    smooth = synth.smooth_frames_u8(1, 4, 128, 128, seed=7)[0]
    return (("jitter", jit, 16, 2000), ("steady", steady, 8, 2000), ("rolled", R.rolled_noise(_shifts(8), 96, 112, seed=1), 8, 2000),
            ("smooth", (smooth.astype(np.float32) / np.float32(255) * np.float32(2) - np.float32(1)).astype(np.float32), 8, 1000))


def test_fit_agrees_with_the_restatement_within_its_own_summation_spread(hip):
    """The tolerance is measured, not guessed: the float64 restatement is evaluated under three summation orders (forward, reverse,
    pairwise) on these inputs, and the kernel -- a fourth order: a lane's blocks in index order, then a butterfly -- may differ from the
    forward one by 16 times the largest spread found, at least 1e-12.  Measured on these clips (printed below): spreads of 0 ..
    1.8e-15 and a kernel 0 .. 1.3e-15 away from the forward order, so the floor of 1e-12 is what holds.  The inlier counts are equal exactly: the
    test asserts first that no block lies within a relative 1e-3 of a round's threshold."""
    from pwstablenet_amd.stream import global_motion
    for name, planes, radius, min_act in _fit_clips():
        h, w = planes.shape[1:]
        d = torch.from_numpy(planes).cuda()
        motion, inl, mv, sad, act = global_motion(d, radius, min_act, return_blocks=True)
        assert motion.dtype == torch.float64 and motion.shape == (planes.shape[0], 4) and inl.dtype == torch.int32 and motion.is_cuda
        blocks = [x.cpu().numpy() for x in (mv, sad, act)]
        if name != "jitter":   # (the live shape's blocks are held to the restatement in the test above)
            assert all(np.array_equal(a, b) for a, b in zip(blocks, R.block_motion(planes, radius))), name
        margins = []
        want, want_inl = R.motion_fit(*blocks, h, w, radius, min_act, "forward", margins)
        assert not margins or min(margins) > 1e-3, (name, min(margins))
        others = [R.motion_fit(*blocks, h, w, radius, min_act, order) for order in ("reverse", "pairwise")]
        nan = np.isnan(want)
        assert all(np.array_equal(np.isnan(m), nan) and np.array_equal(i, want_inl) for m, i in others), name
        spread = max([float(np.nanmax(np.abs(m - want))) for m, _ in others if not nan.all()] + [0.0])
        tol = max(16.0 * spread, 1e-12)
        got = motion.cpu().numpy()
        assert np.array_equal(np.isnan(got), nan), name
        err = float(np.nanmax(np.abs(got - want))) if not nan.all() else 0.0
        print(name, "spread of the restatement's orders", spread, "kernel against forward", err, "tolerance", tol,
              "smallest margin", min(margins) if margins else None, "inliers", want_inl.tolist())
        assert err <= tol, (name, err, tol)
        assert np.array_equal(inl.cpu().numpy(), want_inl), name
        assert got[0].tolist() == [1.0, 0.0, 0.0, 0.0] and int(inl[0]) == 0
        again = global_motion(d, radius, min_act, return_blocks=True)
        assert all(torch.equal(a, b) or (a.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64)))
                   for a, b in zip(again, (motion, inl, mv, sad, act))), name
        if name == "jitter":
            exp = R.expected_motion(R.planted_path(6, seed=11, jitter=True))
            assert np.rad2deg(np.abs(np.arctan2(got[1:, 1], got[1:, 0]) - exp[1:, 0])).max() <= 0.1
            assert np.abs(got[1:, 2:] - exp[1:, 1:]).max() <= 0.25
        if name == "rolled":   # inside the range: the planted shift exactly; on the rim and beyond it: NaN
            sh = _shifts(8)
            for k in (1, 2, 7):
                assert np.abs(got[k] - [1.0, 0.0, sh[k][0], sh[k][1]]).max() <= 1e-9
            assert np.isnan(got[3:7]).all() and not inl[3:7].any()


def test_motion_errors(hip):
    from pwstablenet_amd.stream import block_motion, global_motion
    x = torch.zeros((3, 64, 64), device="cuda")
    for fn in (block_motion, global_motion):
        for bad in (x.transpose(1, 2)[:, :, ::2], x[:, ::2], x.double(), x.half(), x[0], x.to(torch.int32), x.cpu().numpy()):
            with pytest.raises(ValueError):
                fn(bad, 8)
        for radius in (0, 17, -1):
            with pytest.raises(ValueError, match="radius"):
                fn(x, radius)
        with pytest.raises(ValueError, match="no 16 x 16 block"):
            fn(torch.zeros((2, 47, 64), device="cuda"), 16)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x.cpu(), 8)
    L = hip.lib()
    mv = torch.zeros((3, 3, 3, 2), dtype=torch.int16, device="cuda")
    sad = torch.zeros((3, 3, 3, 5), dtype=torch.int32, device="cuda")
    act = torch.zeros((3, 3, 3), dtype=torch.int32, device="cuda")
    motion, inl = torch.zeros((3, 4), dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    P = hip.ptr
    assert L.pws_block_motion(P(x), 3, 64, 64, 0, P(mv), P(sad), P(act), None) == -22 and b"radius" in L.pws_last_error()
    assert L.pws_block_motion(P(x), 3, 64, 64, 17, P(mv), P(sad), P(act), None) == -22 and b"radius" in L.pws_last_error()
    assert L.pws_block_motion(P(x), 3, 31, 64, 8, P(mv), P(sad), P(act), None) == -22 and b"no 16 x 16 block" in L.pws_last_error()
    assert L.pws_block_motion(P(x), -1, 64, 64, 8, P(mv), P(sad), P(act), None) == -22 and b"bad shape" in L.pws_last_error()
    assert L.pws_block_motion(None, 3, 64, 64, 8, P(mv), P(sad), P(act), None) == -22 and b"NULL" in L.pws_last_error()
    assert L.pws_block_motion(P(x), 3, 64, 64, 8, P(mv), None, P(act), None) == -22 and b"NULL" in L.pws_last_error()
    assert L.pws_block_motion(P(x), 3, 64, 64, 8, hip.ctypes.c_void_p(mv.data_ptr() + 2), P(sad), P(act), None) == -22 and b"aligned" in L.pws_last_error()
    assert L.pws_block_motion(None, 0, 64, 64, 8, None, None, None, None) == 0
    assert L.pws_motion_fit(P(mv), P(sad), P(act), 3, 64, 64, 0, 2000, P(motion), P(inl), None) == -22 and b"radius" in L.pws_last_error()
    assert L.pws_motion_fit(P(mv), P(sad), P(act), 3, 64, 20, 8, 2000, P(motion), P(inl), None) == -22 and b"no 16 x 16 block" in L.pws_last_error()
    assert L.pws_motion_fit(P(mv), P(sad), P(act), 3, 64, 64, 8, 2000, None, P(inl), None) == -22 and b"NULL" in L.pws_last_error()
    assert L.pws_motion_fit(P(mv), P(sad), P(act), 3, 64, 64, 8, 2000, hip.ctypes.c_void_p(motion.data_ptr() + 4), P(inl), None) == -22
    assert b"aligned" in L.pws_last_error()
    assert L.pws_motion_fit(None, None, None, 0, 64, 64, 8, 2000, None, None, None) == 0
    assert L.pws_block_motion(P(x), 3, 64, 64, 8, P(mv), P(sad), P(act), None) == 0
    assert L.pws_motion_fit(P(mv), P(sad), P(act), 3, 64, 64, 8, 2000, P(motion), P(inl), None) == 0
    torch.cuda.synchronize()
    assert torch.isnan(motion[1:]).all() and motion[0].tolist() == [1.0, 0.0, 0.0, 0.0]   # a flat plane: no block counts
