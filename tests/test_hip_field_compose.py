"""GPU tests of the composition kernel (csrc/field_compose.hip; functional.compose_fields, C: pws_field_compose) against the float64
restatement tests/path_ref.py.

Lattices (2, 2) (the smallest: one cell, everything else is continuation), (3, 5) (odd width: a lane with one node, rows at 8 mod 16 bytes),
(17, 130) (crosses the 128-node wave segment: two column chunks; five row groups with a partial last one) and (256, 256), the live shape;
three frames each, a 640 x 360 frame.

Values, against float64, per value: 2^-22 W max|corner| with W = (|1 - lx| + |lx|)(|1 - ly| + |ly|) -- the blend's three float32 roundings under
the absolute sum of its weights -- plus 2^-16 max|corner difference| -- one float32 rounding of each lattice coordinate, which is at most
256 (path_ref.compose64 returns the bound).  Where the definition promises a copy (identity rows, rows that are not finite) the bound is 0.
Counts: exact, except at nodes whose float64 coordinate lies within that tolerance (in pixels, plus one float32 rounding of the
un-normalised coordinate) of a coverage threshold; their share is asserted below 1 % on the reference alone."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import path_ref as P  # noqa: E402

FRAME = (360, 640)
LATTICES = [(2, 2), (3, 5), (17, 130), (256, 256)]
IDS = ["%dx%d" % s for s in LATTICES]
T = 3
CAP = 0.01


def _seed(lat):
    return lat[0] * 7 + lat[1]


@functools.lru_cache(maxsize=None)
def field_of(lat, scale=1.0):
    f = P.make_field((T,) + lat + (2,), _seed(lat), scale=scale)
    f.setflags(write=False)
    return f


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def similarity(deg, scale, tx, ty):
    c, s = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    return [c, -s, tx, s, c, ty]


def _check(field, d, what, counts=True):
    """compose_fields against compose64 within the bound, for both coordinate conventions' counts; returns the kernel's output."""
    from pwstablenet_amd import functional as PF
    d = np.asarray(d, np.float64)
    want, tol = P.compose64(field, d, FRAME, return_terms=True)
    field_d, d_d = dev(field), dev(d)
    got_d = PF.compose_fields(field_d, d_d, FRAME)
    got = got_d.cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    worst = float((err - tol).max())
    print("%s %s: largest error %.3g, largest bound %.3g, largest error over its bound %.3g" % (
        what, field.shape, err.max(), tol.max(), float((err / np.maximum(tol, 1e-300)).max())))
    assert worst <= 0.0, (what, worst)
    if counts:
        for ac in (False, True):
            for mode, m in (("bilinear", 0), ("bicubic", 1)):
                lo, hi, share = P.uncovered_bounds(want, tol, FRAME, ac, m)
                assert share <= CAP, (what, share)   # (the reference alone)
                out, unc = PF.compose_fields(field_d, d_d, FRAME, align_corners=ac, mode=mode, return_uncovered=True)
                assert torch.equal(out, got_d) and unc.dtype == torch.int32 and tuple(unc.shape) == (field.shape[0],)
                unc = unc.cpu().numpy()
                print("   ac=%s %s: uncovered %s, float64 %s .. %s" % (ac, mode, unc, lo, hi))
                assert (lo <= unc).all() and (unc <= hi).all(), what
    return got_d


@pytest.mark.parametrize("lat", LATTICES, ids=IDS)
def test_identity_is_a_bit_equal_copy(hip, lat):
    from pwstablenet_amd import functional as PF
    field = np.array(field_of(lat))
    field[0, 0, 0, 0] = -0.0
    field[1, lat[0] - 1, lat[1] - 1, 1] = np.nan   # (a copy does not read a value's meaning)
    field_d = dev(field)
    d = torch.tensor([P.IDENTITY] * T, dtype=torch.float64, device="cuda")
    got, unc = PF.compose_fields(field_d, d, FRAME, return_uncovered=True)
    assert got.data_ptr() != field_d.data_ptr() and torch.equal(got.view(torch.int32), field_d.view(torch.int32))
    want = P.uncovered_bounds(field.astype(np.float64), np.zeros(field.shape), FRAME, False, 0)
    assert (want[0] <= unc.cpu().numpy()).all() and (unc.cpu().numpy() <= want[1]).all() and int(unc[1]) >= 1   # (the NaN node is not covered)
    out = torch.empty_like(field_d)
    assert PF.compose_fields(field_d, d, FRAME, out=out) is out and torch.equal(out.view(torch.int32), field_d.view(torch.int32))


@pytest.mark.parametrize("lat", LATTICES, ids=IDS)
def test_whole_node_shift_of_an_affine_field(hip, lat):
    """An affine field under a shift by whole nodes is the same affine field of the shifted nodes -- also beyond the lattice, where the
    continuation is linear: against the closed form, not only against the restatement."""
    fh, fw = lat
    u, v = np.meshgrid(np.linspace(-1, 1, fw), np.linspace(-1, 1, fh))
    F = np.stack([0.9 * u + 0.1 * v + 0.02, -0.05 * u + 1.1 * v - 0.01], -1).astype(np.float32)
    field = np.stack([F] * T)
    kx, ky = (FRAME[1] - 1) / (fw - 1), (FRAME[0] - 1) / (fh - 1)
    shifts = [(1, 0), (-2, 1), (0, -3)]
    d = [[1.0, 0.0, a * kx, 0.0, 1.0, b * ky] for a, b in shifts]
    got = _check(field, d, "shift", counts=False).cpu().numpy().astype(np.float64)
    _, tol = P.compose64(field, np.array(d), FRAME, return_terms=True)
    for t, (a, b) in enumerate(shifts):
        us, vs = u + a * 2.0 / (fw - 1), v + b * 2.0 / (fh - 1)
        closed = np.stack([0.9 * us + 0.1 * vs + 0.02, -0.05 * us + 1.1 * vs - 0.01], -1)
        # (the float32 field's own rounding of the affine function, carried by the continuation's weights: 2^-24 W |F|, inside the bound's first term)
        assert (np.abs(got[t] - closed) <= tol[t] + 2.0 ** -22 * (1 + abs(a) + abs(b)) ** 2).all(), (t, np.abs(got[t] - closed).max())


@pytest.mark.parametrize("lat", LATTICES, ids=IDS)
def test_rotation_and_scale_on_a_smooth_field(hip, lat):
    d = [similarity(5.0, 1.05, 0.0, 0.0), similarity(-5.0, 1.0 / 1.05, 7.25, -3.5), similarity(0.3, 1.0, -12.0, 4.0)]
    _check(np.array(field_of(lat, 1.04)), d, "rotation")


@pytest.mark.parametrize("lat", LATTICES, ids=IDS)
def test_a_shift_of_a_million_pixels_continues_the_field(hip, lat):
    d = [[1.0, 0.0, 1e6, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0, 1.0, -1e6], similarity(5.0, 1.05, -1e6, 1e6)]
    got = _check(np.array(field_of(lat)), d, "far")
    assert float(got[0, ..., 0].min()) > 1e3 and float(got[1, ..., 1].max()) < -1e3   # every node is continuation: far outside [-1, 1]


@pytest.mark.parametrize("lat", LATTICES, ids=IDS)
def test_rows_that_are_not_finite_keep_the_field(hip, lat):
    from pwstablenet_amd import functional as PF
    field_d = dev(field_of(lat))
    nan, inf = float("nan"), float("inf")
    d = torch.tensor([[nan, 0.0, 0.0, 0.0, 1.0, 0.0], [1.0, 0.0, inf, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0, 1.0, -1e300]], dtype=torch.float64, device="cuda")
    got = PF.compose_fields(field_d, d, FRAME)
    assert torch.equal(got.view(torch.int32), field_d.view(torch.int32))
    # a row that is finite but wild: its frame's result does not depend on what the neighbouring frames hold
    d = torch.tensor([list(P.IDENTITY), [1e30, -1e30, 1e30, 1e30, 1e30, -1e30], list(P.IDENTITY)], dtype=torch.float64, device="cuda")
    other = torch.full((T,) + lat + (2,), 5.0, device="cuda")
    other[1] = field_d[1]
    a, b = PF.compose_fields(field_d, d, FRAME), PF.compose_fields(other, d, FRAME)
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _call(hip, field, n, fh, fw, d, out, unc=None, h0=360, w0=640, margin=0):
    p = lambda t: ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else None   # noqa: E731
    return hip.lib().pws_field_compose(p(field), n, fh, fw, p(d), p(out), h0, w0, 0, margin, p(unc), hip.current_stream())


def test_bad_arguments(hip):
    from pwstablenet_amd import functional as PF
    EINVAL = -22
    n, fh, fw = 2, 8, 12
    field = torch.zeros((n + 1, fh, fw, 2), device="cuda")
    d = torch.tensor([P.IDENTITY] * n, dtype=torch.float64, device="cuda")
    out = torch.full((n, fh, fw, 2), 7.0, device="cuda")
    assert _call(hip, field, n, fh, fw, d, field) == EINVAL                                # exact aliasing
    assert _call(hip, field, n, fh, fw, d, field.data_ptr() + fh * fw * 8) == EINVAL        # out = field + one frame
    assert _call(hip, field.data_ptr() + fh * fw * 8, n, fh, fw, d, field) == EINVAL        # and the other way round
    assert b"overlap" in hip.lib().pws_last_error()
    assert _call(hip, field, n, 1, fw, d, out) == EINVAL and _call(hip, field, n, fh, 1, d, out) == EINVAL
    assert _call(hip, field, n, fh, fw, d, out, h0=1) == EINVAL and _call(hip, field, n, fh, fw, d, out, w0=1) == EINVAL
    assert _call(hip, None, n, fh, fw, d, out) == EINVAL and _call(hip, field, n, fh, fw, None, out) == EINVAL
    assert _call(hip, field, n, fh, fw, d, None) == EINVAL and _call(hip, field, -1, fh, fw, d, out) == EINVAL
    unc = torch.full((n,), -3, device="cuda", dtype=torch.int32)
    assert _call(hip, field, n, fh, fw, d, out, unc, margin=-1) == EINVAL
    assert _call(hip, field, n, fh, fw, d.data_ptr() + 4, out) == EINVAL and b"aligned" in hip.lib().pws_last_error()
    # n = 0: nothing is launched, nothing is written (NULL pointers are fine)
    assert _call(hip, field, 0, fh, fw, d, out, unc) == 0 and _call(hip, None, 0, fh, fw, None, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((unc == -3).all())
    empty = PF.compose_fields(field[:0], d[:0], FRAME, return_uncovered=True)
    assert tuple(empty[0].shape) == (0, fh, fw, 2) and tuple(empty[1].shape) == (0,)
    # the Python layer's own refusals
    for bad_d in (d.float(), d.cpu(), d[:1], d[:, :5]):
        with pytest.raises(ValueError, match="d must"):
            PF.compose_fields(field[:n], bad_d, FRAME)
    with pytest.raises(ValueError, match="mode"):
        PF.compose_fields(field[:n], d, FRAME, mode="nearest")
    with pytest.raises(ValueError, match="field must"):
        PF.compose_fields(field[:n, :1], d, FRAME)
    with pytest.raises(ValueError, match="2 x 2"):
        PF.compose_fields(field[:n], d, (1, 640))
    with pytest.raises(ValueError, match="out must"):
        PF.compose_fields(field[:n], d, FRAME, out=out[:1])
    with pytest.raises(RuntimeError, match="overlap"):
        PF.compose_fields(field[:n], d, FRAME, out=field[:n])


def test_two_runs_give_the_same_bytes_and_counts(hip):
    from pwstablenet_amd import functional as PF
    field_d = dev(field_of((256, 256), 1.04))
    d = torch.tensor([similarity(5.0, 1.05, 3.0, -2.0)] * T, dtype=torch.float64, device="cuda")
    a, ua = PF.compose_fields(field_d, d, FRAME, return_uncovered=True)
    b, ub = PF.compose_fields(field_d, d, FRAME, return_uncovered=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ua, ub) and int(ua.sum()) > 0
