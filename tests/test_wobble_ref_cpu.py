"""Pins the float64 restatement of wobble suppression (tests/wobble_ref.py) on the CPU: what the filter must leave alone (the rigid part, a
static residual), what it must do (the Gaussian's attenuation of an alternating residual), its behaviour at cuts and unusable taps, and the
float32 sequence's own error on the GPU tests' shapes (printed: the yardstick of tests/test_hip_wobble.py).  Plus the constructor's checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rigid_ref as G  # noqa: E402
import wobble_ref as WR  # noqa: E402

FRAME = WR.FRAME
HW = (24, 40)


def _homography_fields(n, seed=5):
    m = G.make_homographies(n, seed)
    return np.stack([G.field_from_homography(m[t], HW, FRAME) for t in range(n)]), m


def test_weights_and_radius():
    assert [WR.radius(s) for s in (0.1, 1 / 3, 0.34, 0.5, 2, 4.9, 5)] == [1, 1, 2, 2, 6, 15, 15]
    for s in WR.SIGMAS:
        g = WR.weights(s)
        assert g.dtype == np.float32 and len(g) == 2 * WR.radius(s) + 1 and g[WR.radius(s)] == 1 and np.array_equal(g, g[::-1])
        assert (np.diff(g[:WR.radius(s) + 1]) > 0).all()


@pytest.mark.parametrize("sigma", WR.SIGMAS)
def test_exact_homography_fields_come_back(sigma):
    """E is the rounding of F against P alone (two float32 roundings of the same point through two evaluations): the filter averages it, so
    the output stays within that rounding of F."""
    field, m = _homography_fields(12)
    out, removed, unfit = WR.wobble64(field, m, FRAME, sigma)
    ulp = float(np.spacing(np.float32(np.abs(field).max())))
    assert not unfit.any() and np.abs(out - field).max() <= 2 * ulp
    assert removed.max() <= 2 * ulp * max(FRAME) / 2
    out32 = WR.wobble32(field, m, FRAME, sigma)[0]
    assert np.abs(out32.astype(np.float64) - field).max() <= 3 * ulp   # (plus the output's own rounding)


@pytest.mark.parametrize("sigma", WR.SIGMAS)
def test_a_static_residual_comes_back(sigma):
    """F[t] = P[t] + c with c constant in time: S / W = c at every frame, also at the scene's ends (the weights renormalise)."""
    field, m = _homography_fields(20)
    rs = np.random.RandomState(3)
    c = rs.uniform(-0.05, 0.05, HW + (2,))
    shifted = (field.astype(np.float64) + c).astype(np.float32)
    out = WR.wobble64(shifted, m, FRAME, sigma)[0]
    ulp = float(np.spacing(np.float32(np.abs(shifted).max())))
    assert np.abs(out - shifted).max() <= 4 * ulp   # (E carries F's and P's roundings, half an ulp each, frame by frame)
    out32 = WR.wobble32(shifted, m, FRAME, sigma)[0]
    assert np.abs(out32.astype(np.float64) - shifted).max() <= 6 * ulp


@pytest.mark.parametrize("sigma", WR.SIGMAS)
def test_an_alternating_residual_is_attenuated(sigma):
    n, R = 48, WR.radius(sigma)
    field, m = _homography_fields(n)
    P32 = WR.parts(field, m, FRAME)[0].astype(np.float64)
    e = 0.01
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None, None, None]
    wob = (P32 + e * sign).astype(np.float32)
    out = WR.wobble64(wob, m, FRAME, sigma)[0]
    g = WR.weights(sigma).astype(np.float64)
    k = np.arange(-R, R + 1)
    factor = abs(float((g * np.where(k % 2 == 0, 1.0, -1.0)).sum())) / float(g.sum())
    left = np.abs(out - P32)[R:n - R]
    print("sigma %g: an alternating residual keeps %.3g of its amplitude (interior frames)" % (sigma, factor))
    assert np.abs(left - e * factor).max() <= 1e-7
    assert factor < (0.2 if sigma >= 2 else 1.0)


def test_taps_never_cross_a_cut():
    shape = (30, 24, 40)
    field, m = WR.make_inputs(shape)
    cuts = [7, 19]
    whole = WR.wobble64_scenes(field, m, FRAME, 2.0, cuts)
    for a, b in WR.scenes(30, cuts):
        part = WR.wobble64(field[a:b], m[a:b], FRAME, 2.0)
        for x, y in zip(whole, part):
            assert np.array_equal(x[a:b], y)
    assert not np.array_equal(whole[0], WR.wobble64(field, m, FRAME, 2.0)[0])
    # and a frame on its own: S / W = E, so out = P + (F - P)
    one = WR.wobble64(field[:1], m[:1], FRAME, 2.0)[0]
    assert np.abs(one - field[:1]).max() <= float(np.spacing(np.float32(np.abs(field).max())))


def test_unusable_taps_drop_out_and_keep_their_own_value():
    shape = (9, 24, 40)
    field, m = WR.make_inputs(shape)
    field, m = np.array(field), np.array(m)
    field[4, 3, 5, 0] = np.nan
    m[6, 2] = np.inf   # frame 6: not fitted
    for fn in (WR.wobble64, WR.wobble32):
        out, removed, unfit = fn(field, m, FRAME, 2.0)
        assert list(unfit) == [0, 0, 0, 0, 1, 0, 24 * 40, 0, 0] and removed[6] == 0
        got = np.asarray(out, np.float32) if fn is WR.wobble32 else out.astype(np.float32)
        assert np.array_equal(got[6].view(np.int32), field[6].view(np.int32)) and np.array_equal(got[4, 3, 5].view(np.int32), field[4, 3, 5].view(np.int32))
        assert np.isfinite(np.delete(out.reshape(9, -1), 4, 0)).all() and np.isnan(out[4]).sum() == 1
    # ... and as taps they are not there: the neighbours' values are those of a clip in which that node / frame never counted
    out = WR.wobble64(field, m, FRAME, 2.0)[0]
    P32, usable = WR.parts(field, m, FRAME)
    g = WR.weights(2.0).astype(np.float64)
    t, R = 5, 6
    taps = [s for s in range(9) if abs(s - t) <= R and s != 6]
    E = field[taps].astype(np.float64) - P32[taps].astype(np.float64)
    w = np.array([g[s - t + R] for s in taps])
    want = P32[t].astype(np.float64) + np.tensordot(w, E, 1) / w.sum()
    ok = np.ones((24, 40), bool)
    ok[3, 5] = False
    assert np.abs(out[t] - want)[ok].max() <= 1e-15
    taps_n = [s for s in taps if s != 4]
    wn = np.array([g[s - t + R] for s in taps_n])
    want_n = P32[t, 3, 5].astype(np.float64) + np.tensordot(wn, field[taps_n, 3, 5].astype(np.float64) - P32[taps_n, 3, 5].astype(np.float64), 1) / wn.sum()
    assert np.abs(out[t, 3, 5] - want_n).max() <= 1e-15


@pytest.mark.parametrize("shape", WR.SHAPES, ids=["x".join(str(v) for v in s) for s in WR.SHAPES])
def test_float32_sequence_error(shape):
    """Prints the float32 sequence's error against float64 for every shape and sigma of the GPU tests: the yardstick of their bound."""
    field, m = WR.make_inputs(shape)
    parts = WR.parts(field, m, FRAME)
    ulp = float(np.spacing(np.float32(np.abs(field).max())))
    for sigma in WR.SIGMAS:
        o64, r64, u64 = WR.wobble64(field, m, FRAME, sigma, parts)
        o32, r32, u32 = WR.wobble32(field, m, FRAME, sigma, parts)
        err = float(np.abs(o32.astype(np.float64) - o64).max())
        rerr = WR.removed_error_px(field, m, FRAME, sigma, parts, (o64, o32))
        print("%s sigma %g: float32 sequence's error %.3g (ulp of the field's largest magnitude %.3g); removed %.3g .. %.3g px, its error %.3g px"
              % (shape, sigma, err, ulp, r64.min(), r64.max(), rerr))
        assert err <= 4 * ulp and np.array_equal(u64, u32) and not u64.any()
        assert np.abs(r32 - r64).max() <= rerr


def test_white_wobble_is_attenuated_as_predicted():
    field, m, noise = WR.wobbly_clip(48, HW, FRAME, 1e-3, 9)
    sigma, R = 2.0, WR.radius(2.0)
    out = WR.wobble64(field, m, FRAME, sigma)[0]
    clean = field.astype(np.float64) - noise
    before = float(np.sqrt((noise[R:-R] ** 2).mean()))
    after = float(np.sqrt(((out - clean)[R:-R] ** 2).mean()))
    print("white wobble of RMS %.3g: %.3g after sigma %g, ratio %.3f; predicted sqrt(sum g^2) / sum g = %.3f"
          % (before, after, sigma, after / before, WR.expected_attenuation(sigma)))
    assert abs(after / before - WR.expected_attenuation(sigma)) <= 0.02


def test_constructor_checks_wobble():
    torch = pytest.importorskip("torch")
    from pwstablenet_amd.stream import VideoStabilizer
    for bad in (-0.1, 5.5, float("nan"), float("inf"), "much"):
        with pytest.raises(ValueError, match="wobble"):
            VideoStabilizer(torch.nn.Identity(), device="cpu", wobble=bad)
    vs = VideoStabilizer(torch.nn.Identity(), device="cpu")
    assert vs.wobble == 0.0 and vs.wobble_removed is None and vs.wobble_unfit is None
    assert VideoStabilizer(torch.nn.Identity(), device="cpu", wobble=5).wobble == 5.0
    assert VideoStabilizer(torch.nn.Identity(), device="cpu", wobble=0.5).wobble == 0.5
