"""pws_field_homography (csrc/homography.hip) held to float64: the samples bit for bit against the live resize, M against two float64
solvers that share nothing with each other (tests/homography_ref.py: ``fit``, the restatement, and ``fit_independent``), the bounds to a
derived float32 tolerance, the frames without a fit, batch independence and the C entry point's refusals -- at the minimum frame, odd
frames and large ones, on fields down to 2 x 2 and 1 x 256.  tests/test_homography_ref_cpu.py pins the instruments: every fit entry of
the table has pivot ratios >= 0.59, at most 8 Gauss-Newton steps and two solvers within 1e-12 / 16 of each other, so every gate below
is its floor, 1e-12; a restatement that stops two steps early (2.8e-12 at least) or loses one lattice point (4.3e-5 at least) misses it.

Measured on an MI355X [largest distance; largest share of its gate]:
  fit, 125 entries      kernel to fit [4.7e-16; 0.0005], kernel to fit_independent [6.1e-14, which is fit's own distance there; 0.061]
  first built, 10       kernel to fit [5.0e-16; 0.0002], kernel to fit_independent [1.5e-12 = the spread there; 0.0625 = 1 / 16]
  bounds, 125 entries   [1.7e-4 pixels at 2160 x 3840; 0.39]
  near entries          spread 1e-5, where M's entries reach 1e5 [2.9e-11 to fit; 0.13], near-line [1.9e-12 to fit; 0.035]
The kernel needed no change but the two alignment checks of its entry point: it follows the restatement step for step."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_ref as R  # noqa: E402

LIVE = (360, 640)      # the streaming frame of tests/test_hip_auto_crop.py, with 256 x 256 fields


def _run(fields, frame_hw):
    """field_homography on (n, fh, fw, 2) float32 numpy fields, n <= 8: M (n, 3, 3) float64, bounds (n, 4), pts (n, 400, 2), as numpy."""
    from pwstablenet_amd.stream import field_homography
    assert len(fields) <= 8
    M, bounds, pts = field_homography(torch.from_numpy(np.ascontiguousarray(fields)).cuda(), frame_hw, return_points=True)
    assert (M.dtype, bounds.dtype, pts.dtype) == (torch.float64, torch.float32, torch.float32)
    return M.cpu().numpy(), bounds.cpu().numpy(), pts.cpu().numpy()


def _bits(*arrays):
    return [a.view(np.int64 if a.dtype == np.float64 else np.int32) for a in arrays]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(*a), _bits(*b)))


def _all_nan(M, bounds):
    return bool(np.isnan(M).all() and np.isnan(bounds).all())


@functools.lru_cache(maxsize=None)
def _entry(frame_hw, field_hw):
    """One launch of the table (the five families) and its references, shared by the fit and the bounds tests."""
    M, bounds, pts = _run(R.case_fields(frame_hw, field_hw), frame_hw)
    _, _, p2 = R.lattice(frame_hw)
    refs = [(R.fit(p.astype(np.float64), p2), R.fit_independent(p.astype(np.float64), p2)) for p in pts]
    return M, bounds, pts, refs


def _check_fit(M, p1, p2, what):
    """The gate of the fit: 16 x the spread of the two references on these very samples, at least 1e-12 (tests/test_hip_motion.py's rule:
    the kernel sums in another order than numpy); against both references; m33 exactly 1.  Returns (distance, share of the gate)."""
    ref, ind = R.fit(p1, p2), R.fit_independent(p1, p2)
    assert ref is not None and np.isfinite(M).all() and M[2, 2] == 1.0, what
    spread = float(np.abs(ref - ind).max())
    gate = max(16.0 * spread, 1e-12)
    d_ref, d_ind = float(np.abs(M - ref).max()), float(np.abs(M - ind).max())
    print(what, "kernel to fit %.3g, to fit_independent %.3g, spread %.3g, gate %.3g" % (d_ref, d_ind, spread, gate))
    assert d_ref <= gate and d_ind <= gate, (what, d_ref, d_ind, gate)
    return d_ref, d_ind, max(d_ref, d_ind) / gate


@pytest.mark.parametrize("frame_hw,field_hw", R.CASES)
def test_samples_are_the_live_resize_bit_for_bit(hip, frame_hw, field_hw):
    """Odd frames (h0 / 2 and w0 / 2 as integers), the minimum frame (the lattice on row 0 and column 0), and small and non-square fields
    (the y1 / x1 clamps, more lattice points than nodes)."""
    from pwstablenet_amd import functional as PF
    g = torch.Generator().manual_seed(frame_hw[0] + field_hw[1])
    field = (torch.rand((2,) + field_hw + (2,), generator=g) * 2 - 1)
    _, _, pts = _run(field.numpy(), frame_hw)
    up = PF.upsample_bilinear2d(field.cuda().permute(0, 3, 1, 2).contiguous(), frame_hw).permute(0, 2, 3, 1)
    r, c, _ = R.lattice(frame_hw)
    want = up[:, torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda(), :]
    assert pts.shape == (2, 400, 2) and torch.equal(torch.from_numpy(pts), want.cpu())


@pytest.mark.parametrize("frame_hw,field_hw", R.CASES)
def test_fit_matches_both_float64_solvers(hip, frame_hw, field_hw):
    """From the kernel's own samples, so the resize's rounding is no part of the comparison."""
    M, _, pts, _ = _entry(frame_hw, field_hw)
    _, _, p2 = R.lattice(frame_hw)
    for k, name in enumerate(R.FAMILIES):
        _check_fit(M[k], pts[k].astype(np.float64), p2, "%s %s %s:" % (frame_hw, field_hw, name))


def test_fit_of_the_replaced_entries_as_first_built(hip):
    """The ten entries that left the table because the restatement itself stops up to 1.5e-12 short of the minimiser there (up to 11
    Gauss-Newton steps: the slowest fits there are), under the gate their own spread gives."""
    for frame_hw, field_hw, name in R.REPLACED:
        M, _, pts = _run(R.first_built(field_hw, name)[None], frame_hw)
        _check_fit(M[0], pts[0].astype(np.float64), R.lattice(frame_hw)[2], "first built %s %s %s:" % (frame_hw, field_hw, name))


@pytest.mark.parametrize("frame_hw,field_hw", R.CASES)
def test_bounds_match_the_restatement_to_float32_roundings(hip, frame_hw, field_hw):
    """Derived, not measured: the kernel's M is within 1e-12 of the restatement's, so a corner is the same float64 to 1e-11 and the same
    float32 but where its rounding falls the other way, one float32 spacing of the corner, which the map to pixels scales by h0 / 2 or w0 / 2;
    the bound itself is stored with one more float32 rounding.  The strong family at 300 x 600 has its horizon nearest the corners."""
    M, bounds, _, refs = _entry(frame_hw, field_hw)
    h0, w0 = frame_hw
    worst = 0.0
    for k, name in enumerate(R.FAMILIES):
        c = R.corners(refs[k][0])
        want = R.bounds(refs[k][0], frame_hw)
        assert np.isfinite(bounds[k]).all() and np.isfinite(want).all()
        corner_ulp = [max(R.ulp32(c[0, 1]), R.ulp32(c[3, 1])), max(R.ulp32(c[1, 1]), R.ulp32(c[2, 1])),      # top, bottom
                      max(R.ulp32(c[0, 0]), R.ulp32(c[1, 0])), max(R.ulp32(c[2, 0]), R.ulp32(c[3, 0]))]      # left, right
        tol = np.array([corner_ulp[j] * (h0, h0, w0, w0)[j] / 2 + R.ulp32(want[j]) for j in range(4)])
        err = np.abs(bounds[k].astype(np.float64) - want)
        print(frame_hw, field_hw, name, "bounds", bounds[k], "error", err, "tolerance", tol)
        assert np.all(err <= tol), (name, err, tol)
        worst = max(worst, float((err / tol).max()))
    print(frame_hw, field_hw, "largest share of the bounds' tolerance %.3g" % worst)


@functools.lru_cache(maxsize=None)
def _fitted_pair():
    return R.family_field("projective", (256, 256), 1.0), R.family_field("strong", (256, 256), 2.0)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_frames_without_a_fit_are_nan_and_their_neighbours_untouched(hip, bad):
    """No spread (constant, 1e-8), no rank (line, x-only, parabola: a Cholesky refusal in the DLT) and a NaN or Inf at a node that the
    resize reads: all 9 + 4 outputs NaN, between two fitted frames that equal their single-frame launches bit for bit."""
    a, b = _fitted_pair()
    poisoned = a.copy()
    node = sorted(R.sample64(a, LIVE)[1])[777]
    poisoned[node[0], node[1], 0] = bad
    nofit = R.nofit_fields()
    fields = np.stack([a] + [nofit[k] for k in ("constant", "spread", "line", "x_only", "parabola")] + [poisoned, b])
    M, bounds, pts = _run(fields, LIVE)
    _, _, p2 = R.lattice(LIVE)
    for k in range(1, 7):
        assert _all_nan(M[k], bounds[k]), k
        with np.errstate(invalid="ignore"):
            assert R.fit(pts[k].astype(np.float64), p2) is None, k      # and the restatement refuses the kernel's samples too
    assert np.isfinite(pts[1:6]).all() and not np.isfinite(pts[6]).all()
    for k, f in ((0, a), (7, b)):
        alone = _run(f[None], LIVE)
        assert np.isfinite(M[k]).all() and np.isfinite(bounds[k]).all()
        assert _same_bits((M[k], bounds[k], pts[k]), (alone[0][0], alone[1][0], alone[2][0])), k


@pytest.mark.parametrize("field_hw", [(1, 256), (256, 1)])
def test_a_single_row_or_column_has_no_fit(hip, field_hw):
    """The identity on one row holds one value of y: the samples lie on a line."""
    M, bounds, pts = _run(np.stack([R.family_field("identity", field_hw)] * 2), LIVE)
    assert _all_nan(M, bounds) and np.isfinite(pts).all()
    assert len(np.unique(pts[0, :, 0 if field_hw[1] == 1 else 1])) == 1


def test_near_entries_are_fitted(hip):
    """A spread of 1e-5 and a line opened by 1e-3: finite, and within the fit's gate."""
    near = R.near_fields()
    M, bounds, pts = _run(np.stack([near["spread"], near["line"]]), LIVE)
    _, _, p2 = R.lattice(LIVE)
    for k, name in enumerate(("spread", "line")):
        assert np.isfinite(bounds[k]).all()
        _check_fit(M[k], pts[k].astype(np.float64), p2, "near %s:" % name)


def test_nodes_the_resize_does_not_read_are_not_read(hip):
    """Every node outside the set that the 400 samples' taps touch is made NaN: M, bounds and samples keep their bits.  (The float64 set
    is the float32 kernel's: at 360 x 640 on a 256 x 256 field no sample is nearer than 1 / 359 to a node, far beyond float32 rounding.)"""
    a, _ = _fitted_pair()
    nodes = R.sample64(a, LIVE)[1]
    mask = np.ones((256, 256), bool)
    mask[tuple(np.array(sorted(nodes)).T)] = False
    assert 256 * 256 - 1600 <= mask.sum() < 256 * 256 - 400
    holed = a.copy()
    holed[mask] = np.nan
    M, bounds, pts = _run(np.stack([a, holed]), LIVE)
    assert np.isfinite(M).all() and _same_bits((M[0], bounds[0], pts[0]), (M[1], bounds[1], pts[1]))


def test_a_frame_of_a_batch_is_that_frame_alone_and_runs_repeat(hip):
    """257 frames of (5, 7) fields in one launch, the families cycled at a phase per frame and a constant field at every 16th place."""
    from pwstablenet_amd.stream import field_homography
    frame_hw, n = (301, 601), 257
    names = list(R.FAMILIES)
    fields = np.stack([R.nofit_fields((5, 7))["constant"] if k % 16 == 15 else R.family_field(names[k % 5], (5, 7), 0.05 * k, seed=k)
                       for k in range(n)])
    d = torch.from_numpy(fields).cuda()
    first = [x.cpu().numpy() for x in field_homography(d, frame_hw, return_points=True)]
    again = [x.cpu().numpy() for x in field_homography(d, frame_hw, return_points=True)]
    assert _same_bits(first, again)
    for k in range(n):
        alone = [x.cpu().numpy()[0] for x in field_homography(d[k:k + 1], frame_hw, return_points=True)]
        assert _same_bits(alone, [x[k] for x in first]), k
        assert _all_nan(first[0][k], first[1][k]) == (k % 16 == 15), k
    empty = field_homography(d[:0], frame_hw, return_points=True)
    assert [tuple(x.shape) for x in empty] == [(0, 3, 3), (0, 4), (0, 400, 2)]
    assert [x.dtype for x in empty] == [torch.float64, torch.float32, torch.float32] and all(x.is_cuda for x in empty)


def test_entry_point_refuses_bad_arguments_and_launches_nothing(hip):
    L, P, V = hip.lib(), hip.ptr, hip.ctypes.c_void_p
    n, fh, fw, (h0, w0) = 2, 5, 7, (301, 601)
    field = torch.from_numpy(R.case_fields((301, 601), (5, 7))[1:3].copy()).cuda()
    m = torch.full((n * 9 + 1,), float("nan"), dtype=torch.float64, device="cuda")
    bounds = torch.full((n * 4 + 1,), float("nan"), device="cuda")
    pts = torch.full((n * 800 + 2,), float("nan"), device="cuda")

    def refused(text, *args):
        assert L.pws_field_homography(*args, None) == -22 and text in L.pws_last_error(), (text, L.pws_last_error())

    refused(b"bad shape", P(field), -1, fh, fw, h0, w0, P(m), P(bounds), P(pts))
    refused(b"bad shape", P(field), n, 0, fw, h0, w0, P(m), P(bounds), P(pts))
    refused(b"bad shape", P(field), n, fh, 0, h0, w0, P(m), P(bounds), P(pts))
    refused(b"sampling lattice", P(field), n, fh, fw, 299, w0, P(m), P(bounds), P(pts))
    refused(b"sampling lattice", P(field), n, fh, fw, h0, 599, P(m), P(bounds), P(pts))
    refused(b"NULL", None, n, fh, fw, h0, w0, P(m), P(bounds), P(pts))
    refused(b"NULL", P(field), n, fh, fw, h0, w0, None, P(bounds), P(pts))
    refused(b"NULL", P(field), n, fh, fw, h0, w0, P(m), None, P(pts))
    refused(b"aligned", V(field.data_ptr() + 4), n, fh, fw, h0, w0, P(m), P(bounds), P(pts))
    refused(b"aligned", P(field), n, fh, fw, h0, w0, P(m), P(bounds), V(pts.data_ptr() + 4))
    refused(b"aligned", P(field), n, fh, fw, h0, w0, V(m.data_ptr() + 4), P(bounds), P(pts))
    refused(b"aligned", P(field), n, fh, fw, h0, w0, P(m), V(bounds.data_ptr() + 2), P(pts))
    assert L.pws_field_homography(None, 0, fh, fw, h0, w0, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.isnan(m).all() and torch.isnan(bounds).all() and torch.isnan(pts).all()      # nothing was launched
    assert L.pws_field_homography(P(field), n, fh, fw, h0, w0, P(m), P(bounds), None, None) == 0      # pts_out may be NULL
    torch.cuda.synchronize()
    assert torch.isfinite(m[:n * 9]).all() and torch.isfinite(bounds[:n * 4]).all() and torch.isnan(pts).all()
    without = (m.clone(), bounds.clone())
    m.fill_(float("nan")), bounds.fill_(float("nan"))
    assert L.pws_field_homography(P(field), n, fh, fw, h0, w0, P(m), P(bounds), P(pts), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(m[:n * 9].view(torch.int64), without[0][:n * 9].view(torch.int64)) and torch.isnan(m[n * 9:]).all()
    assert torch.equal(bounds[:n * 4], without[1][:n * 4]) and torch.isnan(bounds[n * 4:]).all()
    assert torch.isfinite(pts[:n * 800]).all() and torch.isnan(pts[n * 800:]).all()      # and nothing past the end
