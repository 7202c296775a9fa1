"""GPU tests of the wobble kernel (csrc/field_wobble.hip; functional.wobble_fields, C: pws_field_wobble) against the float64 restatement
tests/wobble_ref.py.

Shapes (n, fh, fw), each at sigma 0.5, 2 and 5 (R = 2, 6, 15): (1, 67, 129) one frame, odd width; (3, 67, 129) fewer frames than any R;
(40, 256, 256) the stabiliser's lattice, two time segments; and n = L-1, L, L+1, 2L+1 at 64 x 130 for the kernel's segment length L = 32
(functional.WOBBLE_SEGMENT = PWS_WOBBLE_SEGMENT; two column chunks, the second one partial).  The frame is 360 x 640; fields are the identity
grid plus a smooth perturbation plus 3 % noise, new in every frame, the homographies differ per frame: residuals of tens of pixels.

Values: the kernel's largest error against float64 is at most test_hip_rigid.py's bound -- 4 x the error of the same sequence in numpy
float32 (wobble_ref.wobble32) on the same inputs, plus 4 ulps of the field's largest magnitude.  Measured on the CPU
(tests/test_wobble_ref_cpu.py prints it): the float32 sequence's error is 6.3e-8 .. 8.4e-8 on every case with more than one frame, 7.5e-9 on
the single frame.  `removed`: within 4 x the float32 sequence's own error in that distance (wobble_ref.removed_error_px, about 4e-5 pixel) of
the float64 value; `unfit` exactly.  On an MI355X the kernel's error EQUALS the float32 sequence's in all 21 cases -- every value is bit-equal
to wobble32's -- and `removed` is off by 2.4e-6 .. 2.2e-5 pixel under tolerances of 0.9e-4 .. 1.8e-4."""
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
import wobble_ref as WR  # noqa: E402

FRAME = WR.FRAME
IDS = ["x".join(str(v) for v in s) for s in WR.SHAPES]


@functools.lru_cache(maxsize=None)
def inputs_of(shape):
    f, m = WR.make_inputs(shape)
    f.setflags(write=False)
    m.setflags(write=False)
    return f, m, WR.parts(f, m, FRAME)


@functools.lru_cache(maxsize=None)
def reference_of(shape, sigma):
    """(wobble64's, wobble32's) results of one case: computed once, shared, read-only."""
    f, m, parts = inputs_of(shape)
    r64, r32 = WR.wobble64(f, m, FRAME, sigma, parts), WR.wobble32(f, m, FRAME, sigma, parts)
    for a in r64 + r32:
        a.setflags(write=False)
    return r64, r32


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the cached inputs are read-only)


def test_the_segment_length_is_the_one_the_shapes_were_chosen_for(hip):
    from pwstablenet_amd import functional as PF
    assert PF.WOBBLE_SEGMENT == WR.SEGMENT == 32 and PF.WOBBLE_MAX_SIGMA == WR.MAX_SIGMA
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pwstable.h")).read()
    assert "#define PWS_WOBBLE_SEGMENT %d\n" % WR.SEGMENT in hdr


@pytest.mark.parametrize("shape", WR.SHAPES, ids=IDS)
def test_values_and_statistics_against_float64(hip, shape):
    from pwstablenet_amd import functional as PF
    field, m, parts = inputs_of(shape)
    field_d, m_d = dev(field), dev(m)
    ulp = float(np.spacing(np.float32(np.abs(field).max())))
    for sigma in WR.SIGMAS:
        (want, rem64, unfit64), (o32, _, _) = reference_of(shape, sigma)
        e32 = float(np.abs(o32.astype(np.float64) - want).max())
        got, rem, unfit = PF.wobble_fields(field_d, m_d, FRAME, sigma, return_stats=True)
        assert got.data_ptr() != field_d.data_ptr() and rem.dtype == torch.float32 and unfit.dtype == torch.int32 and tuple(rem.shape) == (shape[0],)
        got = got.cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - want).max())
        same = float((got.view(np.int32) == o32.view(np.int32)).mean())
        tol = WR.FACTOR * WR.removed_error_px(field, m, FRAME, sigma, parts, (want, o32))
        rerr = float(np.abs(rem.cpu().numpy().astype(np.float64) - rem64).max())
        print("%s sigma=%g: kernel error %.3g, float32 restatement's %.3g, ulp %.3g; %.4f %% of the values bit-equal to the restatement; "
              "removed %.4g .. %.4g px, off by %.3g px (tolerance %.3g)" % (shape, sigma, err, e32, ulp, 100 * same, rem64.min(), rem64.max(), rerr, tol))
        assert err <= WR.FACTOR * e32 + 4 * ulp
        assert rerr <= tol and (shape[0] == 1 or (rem64 > 1).all())
        assert not unfit64.any() and not unfit.cpu().numpy().any()
        # m as (n, 3, 3), `out`, no statistics: the same bytes
        out = torch.empty_like(field_d)
        assert PF.wobble_fields(field_d, m_d.reshape(-1, 3, 3), FRAME, sigma, out=out) is out
        assert np.array_equal(out.cpu().numpy().view(np.int32), got.view(np.int32))
    assert torch.equal(field_d, dev(field))   # the input is left alone


def _special(n=9, fh=67, fw=129):
    """Frame 2: a NaN in M; 4: det M = 0; 6: a horizon across the frame (D = 1 - 1.5 u, beyond it where u > 2/3); NaN nodes in frames 1, 7
    (the last node of a row of odd width) and 8 (the last frame's last node)."""
    field, m = WR.make_inputs((n, fh, fw), seed=3)
    field, m = np.array(field), np.array(m)
    m[2, 4] = np.nan
    m[4] = [1, 2, 3, 2, 4, 6, 0, 0, 1]
    m[6] = [1, 0, 0, 0, 1, 0, 1.5, 0, 1]
    field[1, 3, 5, 0] = np.nan
    field[7, 10, fw - 1, 1] = np.inf
    field[8, fh - 1, fw - 1, 0] = np.nan
    return field, m


@pytest.mark.parametrize("sigma", WR.SIGMAS)
def test_unusable_nodes_keep_the_field_and_drop_out_as_taps(hip, sigma):
    from pwstablenet_amd import functional as PF
    field, m = _special()
    n, fh, fw, _ = field.shape
    # the reference alone: no node lies within 2^-20 (1 +- 2^-10) of the horizon threshold, where float64 orders of operation could disagree
    ratio = G.positions(m[6], (fh, fw), FRAME)[2]
    assert not ((ratio >= G.HORIZON * (1 - 2.0 ** -10)) & (ratio <= G.HORIZON * (1 + 2.0 ** -10))).any()
    parts = WR.parts(field, m, FRAME)
    usable = parts[1]
    want, rem64, unfit64 = WR.wobble64(field, m, FRAME, sigma, parts)
    o32 = WR.wobble32(field, m, FRAME, sigma, parts)[0]
    got, rem, unfit = PF.wobble_fields(dev(field), dev(m), FRAME, sigma, return_stats=True)
    got, rem, unfit = got.cpu().numpy(), rem.cpu().numpy(), unfit.cpu().numpy()
    assert np.array_equal(unfit, unfit64)
    assert list(unfit) == [0, 1, fh * fw, 0, fh * fw, 0, int((~usable[6]).sum()), 1, 1] and 0 < unfit[6] < fh * fw
    assert np.array_equal(got.view(np.int32)[~usable], field.view(np.int32)[~usable])   # F, bit for bit
    assert rem[2] == 0 and rem[4] == 0
    # excluded as taps: the usable nodes agree with the restatement, in which those taps are not there, under the values test's bound.  Its
    # 4 ulps are those of the largest magnitude involved, which here is P's: towards frame 6's horizon P grows (D/Dc falls to 1e-2), the
    # kernel's P may differ from numpy's by one ulp of it (contracted float64 sums), and that residual is a tap of every frame of the clip
    big = max(float(np.abs(field[np.isfinite(field)]).max()), float(np.abs(parts[0][usable]).max()))
    ulp = float(np.spacing(np.float32(big)))
    e32 = float(np.abs(o32.astype(np.float64)[usable] - want[usable]).max())
    err = float(np.abs(got.astype(np.float64)[usable] - want[usable]).max())
    print("sigma=%g: kernel error %.3g on the usable nodes, float32 restatement's %.3g" % (sigma, err, e32))
    assert np.isfinite(got[usable]).all() and err <= WR.FACTOR * e32 + 4 * ulp
    assert np.abs(rem.astype(np.float64) - rem64).max() <= WR.FACTOR * WR.removed_error_px(field, m, FRAME, sigma, parts, (want, o32))


def test_two_runs_give_the_same_bytes(hip):
    from pwstablenet_amd import functional as PF
    shape = WR.SHAPES[-1]
    field, m, _ = inputs_of(shape)
    field_d, m_d = dev(field), dev(m)
    a = PF.wobble_fields(field_d, m_d, FRAME, 5.0, return_stats=True)
    b = PF.wobble_fields(field_d, m_d, FRAME, 5.0, return_stats=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_scene_cuts_equal_the_per_scene_calls(hip):
    from pwstablenet_amd import functional as PF
    shape = WR.SHAPES[-1]   # 65 frames
    field, m, _ = inputs_of(shape)
    field_d, m_d = dev(field), dev(m)
    cuts = [1, 20, 53]   # a scene of one frame, one shorter than R, one of one segment and a frame, one of 12
    whole = PF.wobble_fields(field_d, m_d, FRAME, 2.0, scene_cuts=cuts, return_stats=True)
    for a, b in WR.scenes(shape[0], cuts):
        part = PF.wobble_fields(field_d[a:b], m_d[a:b], FRAME, 2.0, return_stats=True)
        for x, y in zip(whole, part):
            assert torch.equal(x[a:b].view(torch.int32), y.view(torch.int32))
    uncut = PF.wobble_fields(field_d, m_d, FRAME, 2.0)
    assert not torch.equal(uncut, whole[0])
    assert torch.equal(PF.wobble_fields(field_d, m_d, FRAME, 2.0, scene_cuts=torch.tensor(cuts)), whole[0])
    want = WR.wobble64_scenes(field, m, FRAME, 2.0, cuts)[0]
    assert np.abs(whole[0].cpu().numpy().astype(np.float64) - want).max() <= 1e-6


def _call(hip, field, n, fh, fw, m, sigma, out, rem=None, unfit=None):
    p = lambda t: ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else None   # noqa: E731
    return hip.lib().pws_field_wobble(p(field), n, fh, fw, p(m), sigma, 360, 640, p(out), p(rem), p(unfit), hip.current_stream())


def test_bad_arguments(hip):
    from pwstablenet_amd import functional as PF
    EINVAL = -22
    n, fh, fw = 2, 8, 12
    field = torch.zeros((n + 1, fh, fw, 2), device="cuda")
    m = torch.eye(3, device="cuda", dtype=torch.float64).reshape(1, 9).repeat(n, 1)
    out = torch.full((n, fh, fw, 2), 7.0, device="cuda")
    assert _call(hip, field, n, fh, fw, m, 2.0, out) == 0
    assert _call(hip, field, n, fh, fw, m, 2.0, field) == EINVAL                                # in place: the kernel reads neighbours in time
    assert b"overlap" in hip.lib().pws_last_error()
    assert _call(hip, field, n, fh, fw, m, 2.0, field.data_ptr() + fh * fw * 8) == EINVAL     # out = field + one frame: n - 1 frames overlap
    assert _call(hip, field.data_ptr() + fh * fw * 8, n, fh, fw, m, 2.0, field) == EINVAL     # and the other way round
    assert _call(hip, field, 1, fh, fw, m, 2.0, field.data_ptr() + fh * fw * 8) == 0          # adjacent is fine
    assert _call(hip, field, n, 1, fw, m, 2.0, out) == EINVAL                                 # fh = 1
    assert _call(hip, field, n, fh, 1, m, 2.0, out) == EINVAL
    assert _call(hip, None, n, fh, fw, m, 2.0, out) == EINVAL
    assert _call(hip, field, n, fh, fw, None, 2.0, out) == EINVAL
    assert _call(hip, field, n, fh, fw, m, 2.0, None) == EINVAL
    assert _call(hip, field, -1, fh, fw, m, 2.0, out) == EINVAL
    for s in (0.0, -1.0, 5.0001, float("nan"), float("inf")):
        assert _call(hip, field, n, fh, fw, m, s, out) == EINVAL
    assert b"sigma" in hip.lib().pws_last_error()
    assert _call(hip, field, n, fh, fw, m, 5.0, out) == 0 and _call(hip, field, n, fh, fw, m, 1e-3, out) == 0   # the ends of the range
    assert _call(hip, field.data_ptr() + 4, n, fh, fw, m, 2.0, out) == EINVAL                 # alignment
    assert _call(hip, field, n, fh, fw, m, 2.0, out, out.data_ptr() + 2) == EINVAL
    # n = 0: nothing is launched, nothing is written (NULL pointers are fine)
    out.fill_(7.0)
    rem = torch.full((n,), -3.0, device="cuda")
    unfit = torch.full((n,), -3, device="cuda", dtype=torch.int32)
    assert _call(hip, field, 0, fh, fw, m, 2.0, out, rem, unfit) == 0 and _call(hip, None, 0, fh, fw, None, 2.0, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((rem == -3).all()) and bool((unfit == -3).all())
    empty = PF.wobble_fields(field[:0], m[:0], (360, 640), 2.0, return_stats=True)
    assert tuple(empty[0].shape) == (0, fh, fw, 2) and tuple(empty[1].shape) == (0,) and tuple(empty[2].shape) == (0,)
    # a zero field under M = I: E = -P at every frame, a static residual, so the zero field comes back; any frame size
    small = PF.wobble_fields(field[:n], m, (100, 200), 1.0)
    assert float(small.abs().max()) <= 1e-6
    # the Python layer's own refusals
    for s in (0.0, -0.1, 5.5, float("nan"), "wide"):
        with pytest.raises(ValueError, match="sigma"):
            PF.wobble_fields(field[:n], m, (360, 640), s)
    for bad_field, bad_m in [(field[:n].cpu(), m), (field[:n], m.cpu()), (field[:n], m.float()), (field[:n].double(), m), (field[:n], m[:1]),
                             (field[:n], m.reshape(n, 3, 3)[:, :2]), (field[:n, :1], m), (field[:n, ..., :1], m), (field[0], m)]:
        with pytest.raises(ValueError):
            PF.wobble_fields(bad_field, bad_m, (360, 640), 2.0)
    for bad_out in (out.cpu(), out[:1], out.double(), out.permute(0, 2, 1, 3), field[:n], field[1:]):
        with pytest.raises(ValueError):
            PF.wobble_fields(field[:n], m, (360, 640), 2.0, out=bad_out)
    for bad_cuts in ([0], [n], [1, 1], ["x"]):
        with pytest.raises(ValueError, match="scene_cuts"):
            PF.wobble_fields(field[:n], m, (360, 640), 2.0, scene_cuts=bad_cuts)
