"""GPU tests of the rigid-mode kernel (csrc/field_rigid.hip; functional.rigid_fields, C: pws_field_rigid) against the float64 restatement
tests/rigid_ref.py.

Shapes (3, 256, 256, 2), (2, 24, 40, 2) (one partial wave), (1, 2, 2, 2) (the smallest field), (5, 67, 129, 2) (odd width: rows that start
at 8 mod 16 bytes and end in a lane with one node; a partial last row group; two column chunks), the frame 360 x 640.  Fields are the
identity grid plus a smooth perturbation plus 3 % noise; the homographies differ per frame (rigid_ref.make_homographies).

Values: for r below 1 the kernel's largest error against float64 is at most 4 x the error of the same sequence with the blend in numpy
float32 (rigid_ref.rigid32) on the same inputs, plus 4 ulps of the field's largest magnitude.  Measured on the CPU
(tests/test_rigid_ref_cpu.py prints it): the float32 sequence's error is 5.96e-8 on every shape (half an ulp at 1).  At r = 1 the output is
float32(P64) to one ulp.  On an MI355X the kernel's error EQUALS the float32 sequence's in every case (5.96e-08 / 5.96e-08) and at r = 1 every
value is bit-equal to float32(P64).  Residual: within 4 x the float32 sequence's coordinate error (1.9e-5 pixel) of the float64 value."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rigid_ref as G  # noqa: E402

IDS = ["x".join(str(v) for v in s[:3]) for s in G.SHAPES]


@functools.lru_cache(maxsize=None)
def inputs_of(shape):
    f, m = G.make_field(shape, G.seed_of(shape)), G.make_homographies(shape[0], G.seed_of(shape))
    f.setflags(write=False)
    m.setflags(write=False)
    return f, m


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the cached inputs are read-only)


def _ulps_apart(a, b):
    """the distance of two finite float32 arrays in units in the last place (on the ordered integer line of their bit patterns)"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_values_against_float64(hip, shape):
    from pwstablenet_amd import functional as PF
    field, m = inputs_of(shape)
    field_d, m_d = dev(field), dev(m)
    ulp = float(np.spacing(np.float32(np.abs(field).max())))
    for r in (0.25, 0.5, 0.75):
        want, _, unfit64 = G.rigid64(field, m, G.FRAME, r)
        e32 = float(np.abs(G.rigid32(field, m, G.FRAME, r)[0].astype(np.float64) - want).max())
        got, _, unfit = PF.rigid_fields(field_d, m_d, G.FRAME, r, return_stats=True)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print("%s r=%g: kernel error %.3g, float32 restatement's %.3g, ulp %.3g" % (shape, r, err, e32, ulp))
        assert err <= G.FACTOR * e32 + 4 * ulp
        assert not unfit64.any() and not unfit.cpu().numpy().any()
    # r == 1: the homography itself; m as (T, 3, 3), and `out`
    want = G.rigid64(field, m, G.FRAME, 1.0)[0].astype(np.float32)
    out = torch.empty_like(field_d)
    assert PF.rigid_fields(field_d, m_d.reshape(-1, 3, 3), G.FRAME, out=out) is out
    apart = _ulps_apart(out.cpu().numpy(), want)
    print("%s r=1: %.4f %% of the nodes' values are not bit-equal to float32(P64)" % (shape, 100.0 * float((apart != 0).mean())))
    assert apart.max() <= 1


@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_residual(hip, shape):
    from pwstablenet_amd import functional as PF
    field, m = inputs_of(shape)
    field_d, m_d = dev(field), dev(m)
    _, want, _ = G.rigid64(field, m, G.FRAME, 0.5)
    tol = G.FACTOR * G.coordinate_error_px(field, m, G.FRAME)
    _, a, _ = PF.rigid_fields(field_d, m_d, G.FRAME, 0.5, return_stats=True)
    _, b, _ = PF.rigid_fields(field_d, m_d, G.FRAME, 1.0, return_stats=True)   # (the residual does not depend on r)
    _, c, _ = PF.rigid_fields(field_d, m_d, G.FRAME, 0.5, return_stats=True)
    assert a.dtype == torch.float32 and tuple(a.shape) == (shape[0],)
    got = a.cpu().numpy().astype(np.float64)
    print("%s: residual %s px, float64 %s, tolerance %.3g px" % (shape, got, want, tol))
    assert np.abs(got - want).max() <= tol and (want > 1).all()
    assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _special(shape=(4, 67, 129, 2)):
    """Frame 0: a NaN in M; 1: det M = 0; 2: a horizon across the frame (D = 1 - 1.5 u, beyond it where u > 2/3); 3: an ordinary M."""
    field = G.make_field(shape, 3)
    m = G.make_homographies(4, 3)
    m[0, 4] = np.nan
    m[1] = [1, 2, 3, 2, 4, 6, 0, 0, 1]
    m[2] = [1, 0, 0, 0, 1, 0, 1.5, 0, 1]
    return field, m


def test_unfitted_and_invalid_nodes_keep_the_field(hip):
    from pwstablenet_amd import functional as PF
    field, m = _special()
    T, fh, fw, _ = field.shape
    # the reference alone: no node lies within 2^-20 (1 +- 2^-10) of the horizon threshold, where float64 orders of operation could disagree
    for t in (2, 3):
        ratio = G.positions(m[t], (fh, fw), G.FRAME)[2]
        assert not ((ratio >= G.HORIZON * (1 - 2.0 ** -10)) & (ratio <= G.HORIZON * (1 + 2.0 ** -10))).any()
    for r in (0.5, 1.0):
        want, res64, unfit64 = G.rigid64(field, m, G.FRAME, r)
        got, res, unfit = PF.rigid_fields(dev(field), dev(m), G.FRAME, r, return_stats=True)
        got, unfit = got.cpu().numpy(), unfit.cpu().numpy()
        assert unfit.dtype == np.int32 and np.array_equal(unfit, unfit64)
        assert list(unfit[:2]) == [fh * fw] * 2 and 0 < unfit[2] < fh * fw and unfit[3] == 0
        kept = np.stack([~G.positions(m[t], (fh, fw), G.FRAME)[1] for t in range(T)])
        assert np.array_equal(got.view(np.int32)[kept], field.view(np.int32)[kept])   # F, bit for bit
        assert not np.array_equal(got[2][~kept[2]], field[2][~kept[2]])
        assert np.allclose(got[~kept], want[~kept], rtol=1e-6, atol=1e-6)   # (P grows towards the horizon: a relative bound, a few float32 eps)
        res = res.cpu().numpy()
        assert res[0] == 0 and res[1] == 0 and np.abs(res[2:] - res64[2:]).max() <= G.FACTOR * G.coordinate_error_px(field[2:], m[2:], G.FRAME)


def test_nan_in_the_field(hip):
    from pwstablenet_amd import functional as PF
    shape = G.SHAPES[1]
    field, m = (np.array(a) for a in inputs_of(shape))
    clean = PF.rigid_fields(dev(field), dev(m), G.FRAME, 0.5, return_stats=True)[1]
    field[1, 3, 5, 0] = np.nan
    field[0, 23, 39, 1] = np.nan   # (the last node of a frame)
    want = G.rigid64(field, m, G.FRAME, 1.0)[0].astype(np.float32)
    one, r1, _ = PF.rigid_fields(dev(field), dev(m), G.FRAME, 1.0, return_stats=True)
    assert bool(torch.isfinite(one).all()) and _ulps_apart(one.cpu().numpy(), want).max() <= 1   # healed
    half, r5, unfit = PF.rigid_fields(dev(field), dev(m), G.FRAME, 0.5, return_stats=True)
    nan = torch.isnan(half).cpu().numpy()
    assert nan.sum() == 2 and nan[1, 3, 5, 0] and nan[0, 23, 39, 1] and not unfit.cpu().numpy().any()
    res64 = G.rigid64(field, m, G.FRAME, 0.5)[1]
    tol = G.FACTOR * G.coordinate_error_px(field, m, G.FRAME)
    for r in (r1, r5):
        assert bool(torch.isfinite(r).all()) and bool((r <= clean).all()) and np.abs(r.cpu().numpy() - res64).max() <= tol


@pytest.mark.parametrize("shape", [G.SHAPES[0], G.SHAPES[3]], ids=[IDS[0], IDS[3]])
def test_in_place_gives_the_same_bytes(hip, shape):
    from pwstablenet_amd import functional as PF
    field, m = inputs_of(shape)
    for r in (0.5, 1.0):
        field_d, m_d = dev(field), dev(m)
        want, res, unfit = PF.rigid_fields(field_d, m_d, G.FRAME, r, return_stats=True)
        assert want.data_ptr() != field_d.data_ptr() and torch.equal(field_d, dev(field))
        got, res2, unfit2 = PF.rigid_fields(field_d, m_d, G.FRAME, r, out=field_d, return_stats=True)
        assert got is field_d and torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert torch.equal(res.view(torch.int32), res2.view(torch.int32)) and torch.equal(unfit, unfit2)


def test_rigidity_zero_returns_the_field_and_the_statistics(hip):
    """r = 0 is the field bit for bit -- also beyond an overflowing P, where fma(0, inf, F) would be NaN -- with the statistics of any r."""
    from pwstablenet_amd import functional as PF
    field, m = _special()
    m[3] = [1e-40, 0, 0, 0, 1e-40, 0, 0, 0, 1]   # det = Dc = 1e-80: fitted, every node valid; P = (u, v) x 1e40 is infinite in float32
    field_d, m_d = dev(field), dev(m)
    got, res, unfit = PF.rigid_fields(field_d, m_d, G.FRAME, 0.0, return_stats=True)
    assert got.data_ptr() != field_d.data_ptr() and torch.equal(got.view(torch.int32), field_d.view(torch.int32))
    _, res5, unfit5 = PF.rigid_fields(field_d, m_d, G.FRAME, 0.5, return_stats=True)
    assert torch.equal(res.view(torch.int32), res5.view(torch.int32)) and torch.equal(unfit, unfit5) and int(unfit[3]) == 0
    assert bool(torch.isinf(res[3]))


def test_chained_with_the_fit(hip):
    """field_homography -> rigid_fields(r = 1) -> field_homography: the second fit's bounds are the first's to within 4 x the shift the float64
    restatement shows for the same chain (tests/test_rigid_ref_cpu.py prints it: 2.9e-4 pixel), the factor for the float32 sampling of p1.
    Measured on an MI355X: the bounds move by 2.4e-4 pixel, M by 6.0e-7."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.stream import field_homography
    shape = G.SHAPES[0]
    field = inputs_of(shape)[0]
    ref_px, _ = G.refit_shift(field, G.FRAME)
    field_d = dev(field)
    m1, b1 = field_homography(field_d, G.FRAME)
    assert bool(torch.isfinite(b1).all())
    rigid, res, unfit = PF.rigid_fields(field_d, m1, G.FRAME, 1.0, return_stats=True)
    m2, b2 = field_homography(rigid, G.FRAME)
    shift = float((b2.double() - b1.double()).abs().max())
    print("bounds after rigid_fields(r = 1) and a refit move by %.3g pixel (float64 restatement: %.3g); M by %.3g; residual %s px"
          % (shift, ref_px, float((m2 - m1).abs().max()), res.cpu().numpy()))
    assert not unfit.cpu().numpy().any()
    assert shift <= 4 * ref_px


def _call(hip, field, n, fh, fw, m, r, out, res=None, unfit=None):
    p = lambda t: ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else None   # noqa: E731
    return hip.lib().pws_field_rigid(p(field), n, fh, fw, p(m), r, 360, 640, p(out), p(res), p(unfit), hip.current_stream())


def test_bad_arguments(hip):
    from pwstablenet_amd import functional as PF
    EINVAL = -22
    n, fh, fw = 2, 8, 12
    field = torch.zeros((n + 1, fh, fw, 2), device="cuda")
    m = torch.eye(3, device="cuda", dtype=torch.float64).reshape(1, 9).repeat(n, 1)
    out = torch.full((n, fh, fw, 2), 7.0, device="cuda")
    assert _call(hip, field, n, fh, fw, m, 0.5, field) == 0                                   # exact aliasing is allowed
    assert _call(hip, field, n, fh, fw, m, 0.5, field.data_ptr() + fh * fw * 8) == EINVAL     # out = field + one frame: n - 1 frames overlap
    assert b"overlap" in hip.lib().pws_last_error()
    assert _call(hip, field.data_ptr() + fh * fw * 8, n, fh, fw, m, 0.5, field) == EINVAL     # and the other way round
    assert _call(hip, field, n, 1, fw, m, 0.5, out) == EINVAL                                 # fh = 1
    assert _call(hip, field, n, fh, 1, m, 0.5, out) == EINVAL
    assert _call(hip, None, n, fh, fw, m, 0.5, out) == EINVAL
    assert _call(hip, field, n, fh, fw, None, 0.5, out) == EINVAL
    assert _call(hip, field, n, fh, fw, m, 0.5, None) == EINVAL
    assert _call(hip, field, -1, fh, fw, m, 0.5, out) == EINVAL
    for r in (-0.1, 1.5, float("nan")):
        assert _call(hip, field, n, fh, fw, m, r, out) == EINVAL
    assert b"rigidity" in hip.lib().pws_last_error()
    assert _call(hip, field.data_ptr() + 4, n, fh, fw, m, 0.5, out) == EINVAL                 # alignment
    # n = 0: nothing is launched, nothing is written (NULL pointers are fine)
    res = torch.full((n,), -3.0, device="cuda")
    unfit = torch.full((n,), -3, device="cuda", dtype=torch.int32)
    assert _call(hip, field, 0, fh, fw, m, 0.5, out, res, unfit) == 0 and _call(hip, None, 0, fh, fw, None, 0.5, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((res == -3).all()) and bool((unfit == -3).all())
    empty = PF.rigid_fields(field[:0], m[:0], (360, 640), return_stats=True)
    assert tuple(empty[0].shape) == (0, fh, fw, 2) and tuple(empty[1].shape) == (0,) and tuple(empty[2].shape) == (0,)
    # no 600 x 300 restriction of its own: that is the fit's
    small = PF.rigid_fields(field[:n], m, (100, 200), 1.0).cpu().numpy()   # (M = I: P is the node's own output position, 2x/W0 - 1)
    assert np.array_equal(small[0, 0, 0], [-1, -1]) and np.abs(small[1, -1, -1] - [2 * 199 / 200 - 1, 2 * 99 / 100 - 1]).max() <= 1e-7
    # the Python layer's own refusals
    for r in (-0.1, 1.5, float("nan"), "full"):
        with pytest.raises(ValueError):
            PF.rigid_fields(field[:n], m, (360, 640), r)
    for bad_field, bad_m in [(field[:n].cpu(), m), (field[:n], m.cpu()), (field[:n], m.float()), (field[:n].double(), m), (field[:n], m[:1]),
                             (field[:n], m.reshape(n, 3, 3)[:, :2]), (field[:n, :1], m), (field[:n, ..., :1], m), (field[0], m)]:
        with pytest.raises(ValueError):
            PF.rigid_fields(bad_field, bad_m, (360, 640))
    for bad_out in (out.cpu(), out[:1], out.double(), out.permute(0, 2, 1, 3)):
        with pytest.raises(ValueError):
            PF.rigid_fields(field[:n], m, (360, 640), out=bad_out)
