"""CPU tests of rigid warp mode's float64 restatement tests/rigid_ref.py: on exactly rigid fields, against a refit (the bounds rule of
run_video's two-pass paths), that no test input trips the horizon rule, and the float32 sequence's own error, which tests/test_hip_rigid.py
holds the kernel against."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rigid_ref as G  # noqa: E402

IDS = ["x".join(str(v) for v in s[:3]) for s in G.SHAPES]


@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_an_exactly_rigid_field_comes_back(shape):
    """A field generated FROM H (numpy's inverse), with M = H: for every r the output is P to within float32's rounding of it -- two float32
    roundings of float64 values that agree to 1e-15 differ by one ulp at most, and the blend of values one ulp apart lies between them --
    and the residual is at most that one ulp in pixels, the float32 sequence's coordinate granularity."""
    T, fh, fw, _ = shape
    H = G.make_homographies(T, G.seed_of(shape))
    field = np.stack([G.field_from_homography(H[t], (fh, fw), G.FRAME) for t in range(T)])
    ulp = float(np.spacing(np.float32(np.abs(field).max())))
    ulp_px = ulp * max(G.FRAME) / 2
    for r in (0.25, 0.5, 1):
        for fn in (G.rigid64, G.rigid32):
            out, res, unfit = fn(field, H, G.FRAME, r)
            err = float(np.abs(out.astype(np.float64) - field).max())
            print("%s r=%g %s: |out - P| %.3g (ulp %.3g), residual %.3g px (one ulp: %.3g px)" % (shape, r, fn.__name__, err, ulp, res.max(), ulp_px))
            assert err <= ulp and float(res.max()) <= ulp_px and not unfit.any()


def test_refit_returns_m_and_the_bounds_stay():
    """The bounds rule: pass 1 keeps the RAW fit's bounds although pass 2 warps with the adjusted fields.  At r = 1 the adjusted field is M^-1
    sampled at the nodes; the fit reads it between nodes through the resize's bilinear blend, whose error on a homography with perspective
    terms p is about (node spacing)^2 / 8 x 2 p = (2/255)^2 / 8 x 0.04 = 3e-7, plus float32's 6e-8: the refit's M is M to about that, held here
    with a 20 x margin at 1e-5, and the bounds, W0/2 = 320 times that, must stay below 0.5 pixel, the granularity at which auto_crop_window's
    int() can move at all.  Measured: M moves by 6.2e-07 at most, the bounds by 2.9e-04 pixel."""
    shape = G.SHAPES[0]
    px, dm = G.refit_shift(G.make_field(shape, G.seed_of(shape)), G.FRAME)
    print("refit after r = 1 on the noisy %s field: the four bounds move by %.3g pixel at most, M's entries by %.3g" % (shape, px, dm))
    assert dm <= 1e-5
    assert px < 0.5


@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_no_needless_fallback_and_the_float32_error(shape):
    """On the GPU test's inputs no node trips the horizon rule (unfit == 0 for r in (0, 1)), on the reference alone; and the float32
    sequence's largest error against float64, printed per shape for tests/test_hip_rigid.py to quote."""
    T, fh, fw, _ = shape
    field = G.make_field(shape, G.seed_of(shape))
    m = G.make_homographies(T, G.seed_of(shape))
    for t in range(T):
        _, valid, ratio = G.positions(m[t], (fh, fw), G.FRAME)
        assert valid.all() and ratio.min() > 0.9
    for r in (0.25, 0.5, 0.75, 1):
        w64, r64, u64 = G.rigid64(field, m, G.FRAME, r)
        w32, r32, u32 = G.rigid32(field, m, G.FRAME, r)
        assert not u64.any() and not u32.any()
        e32 = float(np.abs(w32.astype(np.float64) - w64).max())
        print("%s r=%g: float32 sequence's error %.3g, residual %.4f px (float32 %.4f), coordinate error %.3g px"
              % (shape, r, e32, r64.max(), r32.max(), G.coordinate_error_px(field, m, G.FRAME)))
        assert e32 <= 4 * np.finfo(np.float32).eps * np.abs(field).max()
        assert np.abs(r32.astype(np.float64) - r64).max() <= G.coordinate_error_px(field, m, G.FRAME)
        if r == 1:
            assert e32 == 0.0   # full rigidity is P itself in both


def test_unfitted_and_beyond_the_horizon_keep_the_field():
    shape = (4, 24, 40, 2)
    field = G.make_field(shape, 3)
    m = G.make_homographies(4, 3)
    m[0, 4] = np.nan
    m[1] = [1, 2, 3, 2, 4, 6, 0, 0, 1]                  # det = 0
    m[2] = [1, 0, 0, 0, 1, 0, 1.5, 0, 1]                # D = 1 - 1.5 u: the horizon crosses the frame at u = 2/3
    for r in (0.5, 1):
        out, res, unfit = G.rigid64(field, m, G.FRAME, r)
        assert np.array_equal(out[:2], field[:2].astype(np.float64)) and list(unfit[:2]) == [24 * 40] * 2 and not res[:2].any()
        u, _ = G.node_uv((24, 40), G.FRAME)
        beyond = 1 - 1.5 * u < G.HORIZON
        assert 0 < beyond.sum() < 40 and unfit[2] == 24 * beyond.sum() and unfit[3] == 0
        assert np.array_equal(out[2][:, beyond], field[2][:, beyond].astype(np.float64))
        assert not np.array_equal(out[2][:, ~beyond], field[2][:, ~beyond].astype(np.float64))
    # a NaN in F: healed at 1, kept below it, never in the residual
    field[3, 3, 5, 0] = np.nan
    clean = G.rigid64(G.make_field(shape, 3), m, G.FRAME, 0.5)[1][3]
    o1, r1, _ = G.rigid64(field, m, G.FRAME, 1)
    o5, r5, _ = G.rigid64(field, m, G.FRAME, 0.5)
    assert np.isfinite(o1[3]).all() and np.isnan(o5[3, 3, 5, 0]) and np.isnan(o5[3]).sum() == 1
    assert np.isfinite(r1[3]) and np.isfinite(r5[3]) and r5[3] <= clean
