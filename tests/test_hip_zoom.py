"""GPU tests of the zoom kernel (csrc/field_zoom.hip; functional.zoom_fields, C: pws_field_zoom) against the float64 restatement
tests/zoom_ref.py.

Shapes (3, 256, 256, 2), (2, 24, 40, 2) (one partial wave), (1, 2, 2, 2) (the smallest field), (5, 67, 129, 2) (odd width: rows that start
at 8 mod 16 bytes and end in a lane with one node; three row groups with a partial last one; two column chunks).  Fields are the identity
grid plus a smooth perturbation plus 3 % noise; windows differ per frame and include the whole frame and the centred half.

Values: the kernel's largest error against float64 is at most 4 x the error of the same operation sequence in numpy float32 on the same
inputs (zoom_ref.zoom32: the coefficients' float32 rounding, the fma chain), plus 4 ulps of the field's largest magnitude.  Measured on the
CPU (tests/test_zoom_ref_cpu.py prints it): the float32 sequence's error is 6.8e-7 .. 8.6e-7 at 256 x 256, at most 3.6e-7 on the small shapes;
on an MI355X the kernel's error EQUALS it in every case (8.64e-07 / 8.64e-07 at 256 x 256).
Counts: between the nodes uncovered in float64 by more than delta and that number plus the nodes within delta of a threshold; delta = 4 x
the float32 sequence's largest coordinate error on the test's field (1.1e-3 pixels at 256 x 256); the share of such nodes is capped at 1 %
on the reference alone (measured: below 0.01 %)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zoom_ref as Z  # noqa: E402

IDS = ["x".join(str(v) for v in s[:3]) for s in Z.SHAPES]


@functools.lru_cache(maxsize=None)
def field_of(shape, scale=1.0):
    f = Z.make_field(shape, Z.seed_of(shape), scale=scale)
    f.setflags(write=False)
    return f


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the cached fields are read-only)


@pytest.mark.parametrize("shape", Z.SHAPES, ids=IDS)
def test_values_against_float64(hip, shape):
    from pwstablenet_amd import functional as PF
    field = field_of(shape)
    field_d = dev(field)
    ulp = float(np.spacing(np.float32(np.abs(field).max())))
    for wins in Z.window_rounds(shape):
        coef = Z.coefficients(wins, Z.FRAME, shape[1:3])
        want = Z.zoom64(field, coef)
        e32 = float(np.abs(Z.zoom32(field, coef).astype(np.float64) - want).max())
        got = PF.zoom_fields(field_d, wins, Z.FRAME).cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("%s: kernel error %.3g, float32 restatement's %.3g, ulp %.3g" % (shape, err, e32, ulp))
        assert err <= Z.FACTOR * e32 + 4 * ulp
    # a tensor of windows, and `out`
    out = torch.empty_like(field_d)
    assert PF.zoom_fields(field_d, torch.tensor(wins, dtype=torch.float64), Z.FRAME, out=out) is out
    assert np.array_equal(out.cpu().numpy(), got)


@pytest.mark.parametrize("shape", Z.SHAPES, ids=IDS)
def test_whole_frame_returns_the_field_bit_for_bit(hip, shape):
    from pwstablenet_amd import functional as PF
    field_d = dev(field_of(shape))
    h0, w0 = Z.FRAME
    got, unc = PF.zoom_fields(field_d, (0, w0, 0, h0), Z.FRAME, return_uncovered=True)
    assert got.data_ptr() != field_d.data_ptr() and torch.equal(got, field_d)
    assert unc.dtype == torch.int32 and tuple(unc.shape) == (shape[0],)


@pytest.mark.parametrize("shape", Z.SHAPES, ids=IDS)
def test_uncovered_counts(hip, shape):
    from pwstablenet_amd import functional as PF
    field = field_of(shape, Z.COVER_SCALE)
    field_d = dev(field)
    wins = Z.window_rounds(shape)[0]
    coef = Z.coefficients(wins, Z.FRAME, shape[1:3])
    for ac in (False, True):
        for mode in ("bilinear", "bicubic"):
            lo, hi, share, delta = Z.count_bounds(field, coef, Z.FRAME, ac, Z.margin(mode))
            assert share <= Z.CAP, share          # (the reference alone)
            assert lo.sum() > 0                    # some nodes do fall outside
            _, unc = PF.zoom_fields(field_d, wins, Z.FRAME, align_corners=ac, mode=mode, return_uncovered=True)
            unc = unc.cpu().numpy()
            print("%s ac=%s %s: uncovered %s, float64 %s .. %s (delta %.3g px)" % (shape, ac, mode, unc, lo, hi, delta))
            assert (lo <= unc).all() and (unc <= hi).all()


def test_nan_is_not_covered(hip):
    from pwstablenet_amd import functional as PF
    shape = Z.SHAPES[1]
    field = np.array(field_of(shape))
    field[1, 3, 5, 0] = np.nan   # (whole-frame window: the NaN reaches its own node and, as 0 * NaN, the neighbours that hold it as a corner)
    h0, w0 = Z.FRAME
    got, unc = PF.zoom_fields(dev(field), (0, w0, 0, h0), Z.FRAME, return_uncovered=True)
    nans = torch.isnan(got).reshape(shape[0], -1).sum(1).cpu().numpy()
    clean = PF.zoom_fields(dev(field_of(shape)), (0, w0, 0, h0), Z.FRAME, return_uncovered=True)[1].cpu().numpy()
    assert nans[0] == 0 and nans[1] >= 1
    nodes_hit = torch.isnan(got).any(-1).reshape(shape[0], -1).sum(1).cpu().numpy()
    assert np.array_equal(unc.cpu().numpy(), clean + nodes_hit)


def test_two_runs_give_the_same_bytes_and_counts(hip):
    from pwstablenet_amd import functional as PF
    shape = Z.SHAPES[0]
    field_d = dev(field_of(shape, Z.COVER_SCALE))
    wins = Z.window_rounds(shape)[0]
    a, ua = PF.zoom_fields(field_d, wins, Z.FRAME, return_uncovered=True)
    b, ub = PF.zoom_fields(field_d, wins, Z.FRAME, return_uncovered=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ua, ub) and int(ua.sum()) > 0


def _call(hip, field, n, fh, fw, coef, out, unc=None):
    p = lambda t: ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else None   # noqa: E731
    return hip.lib().pws_field_zoom(p(field), n, fh, fw, p(coef), p(out), 360, 640, 0, 0, p(unc), hip.current_stream())


def test_bad_arguments(hip):
    from pwstablenet_amd import functional as PF
    EINVAL = -22
    n, fh, fw = 2, 8, 12
    field = torch.zeros((n + 1, fh, fw, 2), device="cuda")
    coef = torch.tensor([[0.0, 1.0, 0.0, 1.0]] * n, device="cuda")
    out = torch.full((n, fh, fw, 2), 7.0, device="cuda")
    assert _call(hip, field, n, fh, fw, coef, field) == EINVAL                       # exact aliasing
    assert _call(hip, field, n, fh, fw, coef, field.data_ptr() + fh * fw * 8) == EINVAL   # out = field + one frame: n - 1 frames overlap
    assert _call(hip, field.data_ptr() + fh * fw * 8, n, fh, fw, coef, field) == EINVAL   # and the other way round
    assert b"overlap" in hip.lib().pws_last_error()
    assert _call(hip, field, n, 1, fw, coef, out) == EINVAL                          # fh = 1
    assert _call(hip, field, n, fh, 1, coef, out) == EINVAL
    assert _call(hip, None, n, fh, fw, coef, out) == EINVAL
    assert _call(hip, field, n, fh, fw, None, out) == EINVAL
    assert _call(hip, field, n, fh, fw, coef, None) == EINVAL
    assert _call(hip, field, -1, fh, fw, coef, out) == EINVAL
    # n = 0: nothing is launched, nothing is written (NULL pointers are fine)
    unc = torch.full((n,), -3, device="cuda", dtype=torch.int32)
    assert _call(hip, field, 0, fh, fw, coef, out, unc) == 0 and _call(hip, None, 0, fh, fw, None, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((unc == -3).all())
    empty = PF.zoom_fields(field[:0], [], (360, 640), return_uncovered=True)
    assert tuple(empty[0].shape) == (0, fh, fw, 2) and tuple(empty[1].shape) == (0,)
    # the Python layer's own refusals
    for bad in [(-1, 640, 0, 360), (0, 641, 0, 360), (0, 640, 5, 5), [(0, 640, 0, 360)] * 3]:
        with pytest.raises(ValueError):
            PF.zoom_fields(field[:n], bad, (360, 640))
    with pytest.raises(ValueError):
        PF.zoom_fields(field[:n], (0, 640, 0, 360), (360, 640), mode="nearest")
    with pytest.raises(ValueError):
        PF.zoom_fields(field[:n, :1], (0, 640, 0, 360), (360, 640))


def test_wild_coefficients_stay_inside_the_field(hip):
    """Coefficients that point far outside (or are NaN) sample the field's edge nodes: the kernel clamps in integers, whatever coef holds."""
    n, fh, fw = 4, 8, 12
    field = dev(Z.make_field((n, fh, fw, 2), 5))
    coef = torch.tensor([[1e30, 1.0, -1e30, 1.0], [float("nan")] * 4, [float("inf"), 0.0, float("-inf"), 0.0], [-3.0, 2.0, 4.0, -1.0]], device="cuda")
    out = torch.empty_like(field)
    assert _call(hip, field, n, fh, fw, coef, out) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[0], field[0, 0:1, fw - 1:fw].expand(fh, fw, 2))   # (x clamps to the last column, y to the first row)
    assert torch.equal(out[1], field[1, 0:1, 0:1].expand(fh, fw, 2))         # NaN -> node 0
    assert torch.equal(out[2], field[2, 0:1, fw - 1:fw].expand(fh, fw, 2))
    want = Z.zoom64(field[3:].cpu().numpy(), coef[3:].cpu().numpy().astype(np.float64))[0]
    assert np.abs(out[3].cpu().numpy() - want).max() < 1e-5
