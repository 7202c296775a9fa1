"""GPU tests of rolling-shutter correction below the stabiliser: the rates kernel (csrc/path_smooth.hip; stream.shutter_rates, C:
pws_shutter_rates) and the row-dependent composition (csrc/field_compose.hip; functional.compose_fields(rates=, rolling_shutter=), C:
pws_field_compose_rows) against the float64 restatement tests/shutter_ref.py.

Composition.  Lattices (2, 2) (one cell), (5, 7) (odd width: a lane with one node; ragged rows), (6, 130) (a second column chunk; rows
that are no multiple of the workgroup's 4) and (256, 256), the live shape; six frames of a 640 x 360 source in two scenes of three, so that
both ends of a scene and a cut in the middle are there; r = 0.8, -1 and 1e-3; rates whose forward and backward rows have opposite signs,
so that a wrong row selection moves a node by pixels.  Values: per value path_ref.compose64's two terms -- 2^-22 W max|corner| + 2^-16
max|corner difference| -- evaluated at the restatement's own sample position: the extra float64 work moves the position by 1e-13 of a
node, nine decades below the float32 rounding of the lattice coordinate that the second term stands for.  Counts: within
path_ref.uncovered_bounds.

Rates.  u = 2^-53.  Kernel and restatement run the same float64 operations in the same order and differ in hypot, atan2, log, cos and sin;
with each of them within 2 ulp = 4u of the true value on either side, two results differ by at most 8u of their size.  ldot = log(s): 8u
from s, which is near 1, plus 8u |ldot|.  wdot: 8u |f|.  The forward translation is copied: 0.  The backward translation (c tx + sn ty) / s:
c and sn carry 8u of their own and 8u |f| <= u from f, the division 8u from s, and the three roundings see inputs that differ, 3u more:
20u (|tx| + |ty|) / s."""
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
import shutter_ref as S  # noqa: E402

FRAME = (360, 640)
LATTICES = [(2, 2), (5, 7), (6, 130), (256, 256)]
IDS = ["%dx%d" % s for s in LATTICES]
RS = [0.8, -1.0, 1e-3]
T, CUT = 6, 3
U = 2.0 ** -53
EINVAL = -22


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def similarity(deg, scale, tx, ty):
    c, s = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    return [c, -s, tx, s, c, ty]


@functools.lru_cache(maxsize=None)
def motion():
    """Six pairs that swing back and forth: 0.5 degree, 0.3 % of scale and (6, 4) pixels, the sign alternating from pair to pair."""
    m = np.zeros((T, 4), np.float64)
    for k in range(T):
        sg = 1.0 if k % 2 else -1.0
        s, th = 1.0 + sg * 0.003, sg * math.radians(0.5)
        m[k] = (s * math.cos(th), s * math.sin(th), sg * 6.0, -sg * 4.0)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def rates():
    r = S.shutter_rates(motion(), [CUT])
    mid = [1, 4]   # the frames with a pair on either side: their two rows disagree in every sign
    assert (np.sign(r[mid, 0]) == -np.sign(r[mid, 1])).all() and (r[mid, 0] != 0).all()
    r.setflags(write=False)
    return r


D = np.array([similarity(2.0, 1.03, 5.0, -3.0), list(P.IDENTITY), similarity(-1.5, 0.98, -8.25, 4.5),
              similarity(0.4, 1.0, 12.0, 0.0), similarity(-3.0, 1.02, 0.0, -9.0), list(P.IDENTITY)])


@functools.lru_cache(maxsize=None)
def field_of(lat):
    f = P.make_field((T,) + lat + (2,), lat[0] * 7 + lat[1], scale=1.04)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def want_of(lat, r):
    return S.compose_rows64(field_of(lat), D, rates(), r, FRAME, return_terms=True)


@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("lat", LATTICES, ids=IDS)
def test_composition_against_float64(hip, lat, r):
    from pwstablenet_amd import functional as PF
    want, tol = want_of(lat, r)
    field_d, d_d, rates_d = dev(field_of(lat)), dev(D), dev(rates())
    got_d = PF.compose_fields(field_d, d_d, FRAME, rates=rates_d, rolling_shutter=r)
    got = got_d.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    err = np.abs(got - want)
    print("%s r %g: largest error %.3g, largest bound %.3g, largest error over its bound %.3g; the correction moves a value by up to %.3g"
          % (lat, r, err.max(), tol.max(), float((err / np.maximum(tol, 1e-300)).max()), np.abs(want - P.compose64(field_of(lat), D, FRAME)).max()))
    assert float((err - tol).max()) <= 0.0
    for ac, mode, m in ((False, "bilinear", 0), (True, "bicubic", 1)):
        lo, hi, share = P.uncovered_bounds(want, tol, FRAME, ac, m)
        out, unc = PF.compose_fields(field_d, d_d, FRAME, align_corners=ac, mode=mode, return_uncovered=True, rates=rates_d, rolling_shutter=r)
        assert torch.equal(out.view(torch.int32), got_d.view(torch.int32)) and unc.dtype == torch.int32 and tuple(unc.shape) == (T,)
        unc = unc.cpu().numpy()
        print("   ac=%s %s: uncovered %s, float64 %s .. %s (undecided share %.4f)" % (ac, mode, unc, lo, hi, share))
        assert (lo <= unc).all() and (unc <= hi).all()


def test_a_wrong_row_selection_would_show(hip):
    """The restatement with the two rows swapped lies far outside the bound: the case above can tell."""
    want, tol = want_of((256, 256), 0.8)
    swapped = S.compose_rows64(field_of((256, 256)), D, rates()[:, ::-1], 0.8, FRAME)
    assert float((np.abs(swapped - want) - tol).max()) > 1e-3


def test_a_steady_pan_is_sheared_in_closed_form(hip):
    """D = I and a pan of v pixels a frame on the identity field: the composed field is x' = x - r v clamp(y / (h0 - 1), -1/2, 1/2), y' = y.
    Against the closed form: the kernel's bound, plus 2^-22 for the float32 identity field's own rounding under weights of at most 4."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as ST
    h0, w0 = FRAME
    for lat in ((7, 9), (256, 256)):
        for r, v in ((0.8, 3.0), (-1.0, -1.25)):
            m = np.tile(np.array([1.0, 0.0, v, 0.0]), (4, 1))
            rates_d = ST.shutter_rates(dev(m))
            assert np.array_equal(rates_d.cpu().numpy(), S.rates(m))
            d = np.tile(np.array(P.IDENTITY), (4, 1))
            field = S.identity_field(4, lat)
            got = PF.compose_fields(dev(field), dev(d), FRAME, rates=rates_d, rolling_shutter=r).cpu().numpy().astype(np.float64)
            _, tol = S.compose_rows64(field, d, S.rates(m), r, FRAME, return_terms=True)
            y, x = np.meshgrid(np.linspace(-0.5 * (h0 - 1), 0.5 * (h0 - 1), lat[0]), np.linspace(-0.5 * (w0 - 1), 0.5 * (w0 - 1), lat[1]), indexing="ij")
            closed = np.stack([(x - r * v * np.clip(y / (h0 - 1), -0.5, 0.5)) / (0.5 * (w0 - 1)), y / (0.5 * (h0 - 1))], -1)
            err = np.abs(got - closed[None])
            print("%s r %g v %g: largest distance from the closed form %.3g (bound %.3g)" % (lat, r, v, err.max(), (tol + 2.0 ** -22).max()))
            assert (err <= tol + 2.0 ** -22).all()
            assert np.abs(got[0, 0, 0, 0] - closed[0, 0, 0]) <= 1e-5 and abs(closed[0, 0, 0] - x[0, 0] / (0.5 * (w0 - 1))) > 1e-3   # a real shear


def test_the_correction_makes_the_frames_rigid_and_the_wrong_sign_does_not(hip):
    """tests/test_shutter_ref_cpu.py's experiment with every composition done by the kernel: the composed identity field read back is p(q)
    itself.  The float64 restatement gives e(+r) = 0.0247 px, e(0) = 0.3485 px, e(-r) = 0.6913 px."""
    from pwstablenet_amd import functional as PF
    hw = (S.SIZE, S.SIZE)

    def compose(field, d, rts, r):
        return PF.compose_fields(dev(field), dev(d), hw, rates=dev(rts), rolling_shutter=r).cpu().numpy()
    e_plus, e_zero, e_minus = S.experiment(compose)
    print("non-rigidity on the device: e(+r) %.4f px, e(0) %.4f px, e(-r) %.4f px, e(+r) / e(0) = %.3f" % (e_plus, e_zero, e_minus, e_plus / e_zero))
    assert e_plus <= 0.5 * e_zero
    assert e_minus > e_zero


def _rows(hip, field, n, fh, fw, d, rates, r, out, unc=None, h0=360, w0=640, margin=0):
    p = lambda t: ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else None   # noqa: E731
    return hip.lib().pws_field_compose_rows(p(field), n, fh, fw, p(d), p(rates), r, p(out), h0, w0, 0, margin, p(unc), hip.current_stream())


@pytest.mark.parametrize("lat", [(5, 7), (256, 256)], ids=["5x7", "256x256"])
def test_bit_equalities(hip, lat):
    from pwstablenet_amd import functional as PF
    fh, fw = lat
    field_d, d_d, rates_d = dev(field_of(lat)), dev(D), dev(rates())
    affine, ua = PF.compose_fields(field_d, d_d, FRAME, return_uncovered=True)
    bits = lambda t: t.view(torch.int32)   # noqa: E731
    # r = 0 with any rates, and all-zero rates with any r: pws_field_compose's bytes, on frames whose D is not the identity
    for r, rt in ((0.0, rates_d), (0.8, torch.zeros_like(rates_d)), (-1.0, torch.zeros_like(rates_d))):
        out, unc = torch.full_like(field_d, 7.0), torch.full((T,), -3, device="cuda", dtype=torch.int32)
        assert _rows(hip, field_d, T, fh, fw, d_d, rt, r, out, unc) == 0
        assert torch.equal(bits(out), bits(affine)) and torch.equal(unc, ua), r
    # the Python layer takes the old entry point when either argument is missing
    assert torch.equal(bits(PF.compose_fields(field_d, d_d, FRAME, rates=rates_d)), bits(affine))
    assert torch.equal(bits(PF.compose_fields(field_d, d_d, FRAME, rolling_shutter=0.8)), bits(affine))
    assert torch.equal(bits(PF.compose_fields(field_d, d_d, FRAME, rates=rates_d, rolling_shutter=0.0)), bits(affine))
    # two runs: the same bytes and counts
    a, ca = PF.compose_fields(field_d, d_d, FRAME, return_uncovered=True, rates=rates_d, rolling_shutter=0.8)
    b, cb = PF.compose_fields(field_d, d_d, FRAME, return_uncovered=True, rates=rates_d, rolling_shutter=0.8)
    assert torch.equal(bits(a), bits(b)) and torch.equal(ca, cb) and not torch.equal(bits(a), bits(affine))
    # an identity frame whose camera moves is not copied (frames 1 and 5); one whose camera stands still is
    assert not torch.equal(bits(a[1]), bits(field_d[1])) and not torch.equal(bits(a[5]), bits(field_d[5]))
    assert torch.equal(bits(affine[1]), bits(field_d[1]))
    still = rates_d.clone()
    still[1] = 0.0
    c = PF.compose_fields(field_d, d_d, FRAME, rates=still, rolling_shutter=0.8)
    assert torch.equal(bits(c[1]), bits(field_d[1])) and torch.equal(bits(c[5]), bits(a[5]))
    # rates that are not finite: the frame keeps its field
    wild = rates_d.clone()
    wild[2, 0, 2] = float("nan")
    wild[2, 1, 0] = float("inf")
    e = PF.compose_fields(field_d, d_d, FRAME, rates=wild, rolling_shutter=0.8)
    assert torch.equal(bits(e[2]), bits(field_d[2])) and torch.equal(bits(e[3]), bits(a[3]))


@functools.lru_cache(maxsize=None)
def _shaky(n):
    rs = np.random.RandomState(200 + n)
    th = np.deg2rad(0.05 + 0.3 * rs.normal(size=n))
    s = 1.0 + 0.002 * rs.normal(size=n)
    m = np.stack([s * np.cos(th), s * np.sin(th), 12.0 + 8.0 * rs.normal(size=n), -5.0 + 8.0 * rs.normal(size=n)], 1)
    m[0] = (np.nan, 0.0, 0.0, 0.0)   # (row 0 is not read)
    if n >= 5:
        m[n // 2] = (np.nan, 0.0, 1.0, np.inf)
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("n", [1, 2, 5, 48, 300])
def test_rates_against_float64(hip, n):
    from pwstablenet_amd.stream import shutter_rates
    m = np.array(_shaky(n))
    got_d = shutter_rates(dev(m))
    assert got_d.is_cuda and got_d.dtype == torch.float64 and tuple(got_d.shape) == (n, 2, 4)
    got, want = got_d.cpu().numpy(), S.rates(m)
    clean = np.where(np.isfinite(m).all(1, keepdims=True), m, np.array([1.0, 0.0, 0.0, 0.0]))
    s = np.hypot(clean[:, 0], clean[:, 1])
    size = (np.abs(clean[:, 2]) + np.abs(clean[:, 3])) / s
    fwd_pair = np.minimum(np.arange(n) + 1, n - 1)   # the pair a row comes from (the ends use their one pair twice; either bound covers both)
    bwd_pair = np.maximum(np.arange(n), min(1, n - 1))
    bound = np.zeros((n, 2, 4))
    for row, pair in ((0, fwd_pair), (1, bwd_pair)):
        bound[:, row, 0] = 8 * U * (1 + np.abs(want[:, row, 0]))
        bound[:, row, 1] = 8 * U * np.abs(want[:, row, 1])
        bound[:, row, 2:] = (20 * U * size[pair])[:, None]
    err = np.abs(got - want)
    print("n %d: largest error %.3g (in units of 2^-53: %.1f), largest error over its bound %.3g"
          % (n, err.max(), err.max() / U, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    assert torch.equal(shutter_rates(dev(m)).view(torch.int64), got_d.view(torch.int64))   # the same bits on every run
    if n == 1:
        assert not got.any()
    else:
        assert np.array_equal(got[0, 0], got[0, 1]) and np.array_equal(got[-1, 0], got[-1, 1])
    if n >= 5:   # the NaN row is the identity row
        c = m.copy()
        c[n // 2] = (1.0, 0.0, 0.0, 0.0)
        assert torch.equal(shutter_rates(dev(c)).view(torch.int64), got_d.view(torch.int64)) and not got[n // 2, 1].any() and not got[n // 2 - 1, 0].any()


def test_rates_stop_at_scene_cuts(hip):
    from pwstablenet_amd.stream import shutter_rates
    m = dev(_shaky(48))
    got = shutter_rates(m, scene_cuts=[20, 21])   # (a scene of one frame between two others)
    for a, b in ((0, 20), (20, 21), (21, 48)):
        assert torch.equal(got[a:b].contiguous().view(torch.int64), shutter_rates(m[a:b].contiguous()).view(torch.int64))
    assert not got[20].any() and torch.equal(got[19, 0], got[19, 1]) and torch.equal(got[21, 0], got[21, 1])
    assert np.abs(got.cpu().numpy() - S.shutter_rates(_shaky(48), [20, 21])).max() <= 1e-13
    assert tuple(shutter_rates(m[:0]).shape) == (0, 2, 4)


def test_bad_arguments(hip):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.stream import shutter_rates
    L, Pt = hip.lib(), hip.ptr
    n, fh, fw = 2, 8, 12
    field = torch.zeros((n + 1, fh, fw, 2), device="cuda")
    d = torch.tensor([P.IDENTITY] * n, dtype=torch.float64, device="cuda")
    rt = torch.ones((n, 2, 4), dtype=torch.float64, device="cuda")
    out = torch.full((n, fh, fw, 2), 7.0, device="cuda")
    unc = torch.full((n,), -3, device="cuda", dtype=torch.int32)
    for r in (0.8, 0.0):   # pws_field_compose's matrix, also where r = 0 hands the call on
        assert _rows(hip, field, n, fh, fw, d, rt, r, field) == EINVAL                                  # exact aliasing
        assert _rows(hip, field, n, fh, fw, d, rt, r, field.data_ptr() + fh * fw * 8) == EINVAL          # out = field + one frame
        assert _rows(hip, field.data_ptr() + fh * fw * 8, n, fh, fw, d, rt, r, field) == EINVAL and b"overlap" in L.pws_last_error()
        assert _rows(hip, field, n, 1, fw, d, rt, r, out) == EINVAL and _rows(hip, field, n, fh, 1, d, rt, r, out) == EINVAL
        assert _rows(hip, field, n, fh, fw, d, rt, r, out, h0=1) == EINVAL and _rows(hip, field, n, fh, fw, d, rt, r, out, w0=1) == EINVAL
        assert _rows(hip, None, n, fh, fw, d, rt, r, out) == EINVAL and _rows(hip, field, n, fh, fw, None, rt, r, out) == EINVAL
        assert _rows(hip, field, n, fh, fw, d, rt, r, None) == EINVAL and _rows(hip, field, -1, fh, fw, d, rt, r, out) == EINVAL
        assert _rows(hip, field, n, fh, fw, d, rt, r, out, unc, margin=-1) == EINVAL
        assert _rows(hip, field, n, fh, fw, d.data_ptr() + 4, rt, r, out) == EINVAL and b"aligned" in L.pws_last_error()
        assert _rows(hip, field, n, fh, fw, d, None, r, out) == EINVAL and b"rates" in L.pws_last_error()
        assert _rows(hip, field, n, fh, fw, d, rt.data_ptr() + 4, r, out) == EINVAL and b"rates" in L.pws_last_error()
        # n = 0: nothing is launched, nothing is written (NULL pointers are fine)
        assert _rows(hip, field, 0, fh, fw, d, rt, r, out, unc) == 0 and _rows(hip, None, 0, fh, fw, None, None, r, None) == 0
    for r in (1.0000001, -1.5, float("nan"), float("inf")):
        assert _rows(hip, field, n, fh, fw, d, rt, r, out) == EINVAL and b"[-1, 1]" in L.pws_last_error()
    m = torch.zeros((5, 4), dtype=torch.float64, device="cuda")
    rates5 = torch.full((5, 2, 4), 7.0, dtype=torch.float64, device="cuda")
    assert L.pws_shutter_rates(None, 5, Pt(rates5), None) == EINVAL and b"NULL" in L.pws_last_error()
    assert L.pws_shutter_rates(Pt(m), 5, None, None) == EINVAL and L.pws_shutter_rates(Pt(m), -1, Pt(rates5), None) == EINVAL
    assert L.pws_shutter_rates(ctypes.c_void_p(m.data_ptr() + 4), 4, Pt(rates5), None) == EINVAL and b"aligned" in L.pws_last_error()
    assert L.pws_shutter_rates(Pt(m), 4, ctypes.c_void_p(rates5.data_ptr() + 4), None) == EINVAL
    assert L.pws_shutter_rates(None, 0, None, None) == 0 and L.pws_shutter_rates(Pt(m), 0, Pt(rates5), None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((unc == -3).all()) and bool((rates5 == 7.0).all())
    assert _rows(hip, field, n, fh, fw, d, rt, 1.0, out) == 0 and _rows(hip, field, n, fh, fw, d, rt, -1.0, out) == 0   # the ends of the range
    torch.cuda.synchronize()
    # the Python layer's own refusals
    for bad in (m.float(), m.cpu(), m[:, :3], m[0], m.cpu().numpy()):
        with pytest.raises(ValueError, match="motion"):
            shutter_rates(bad)
    with pytest.raises(ValueError, match="scene_cuts"):
        shutter_rates(m, scene_cuts=[5])
    for bad in (rt.float(), rt.cpu(), rt[:1], rt[:, :, :3], rt.reshape(n, 8)):
        with pytest.raises(ValueError, match="rates must"):
            PF.compose_fields(field[:n], d, FRAME, rates=bad, rolling_shutter=0.5)
    for bad in (1.5, -1.01, float("nan"), "x", None):
        with pytest.raises(ValueError, match="rolling_shutter"):
            PF.compose_fields(field[:n], d, FRAME, rates=rt, rolling_shutter=bad)
    with pytest.raises(RuntimeError, match="overlap"):
        PF.compose_fields(field[:n], d, FRAME, out=field[:n], rates=rt, rolling_shutter=0.5)
    empty = PF.compose_fields(field[:0], d[:0], FRAME, return_uncovered=True, rates=rt[:0], rolling_shutter=0.5)
    assert tuple(empty[0].shape) == (0, fh, fw, 2) and tuple(empty[1].shape) == (0,)
