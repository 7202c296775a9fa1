"""Float64 restatement of rigid warp mode (functional.rigid_fields, csrc/field_rigid.hip), plus the same operation sequence with the blend and
the residual in numpy float32: the yardstick the GPU tests measure the kernel against (tests/test_hip_rigid.py).

Definition.  M (3 x 3, float64, as field_homography fits it) maps a field VALUE -- normalised source coordinates -- to the output position
u = 2x/W0 - 1, v = 2y/H0 - 1 of the H0 x W0 frame (the reference's convention: no half-pixel term).  Node (i, j) of the fh x fw field stands for
frame pixel x = j (W0-1)/(fw-1), y = i (H0-1)/(fh-1): the pixel at which the warps' align_corners=True resize reads exactly that node.
A = adj(M) (M^-1 up to scale; no division), (X, Y, D) = A (u, v, 1), Dc = A[2][2] (D at u = v = 0), P = (X/D, Y/D) in float64, each rounded
once to float32.  A frame is FITTED when M's nine entries are finite, det M is finite and non-zero and Dc != 0; a node of a fitted frame is
VALID when D/Dc >= 2^-20 (the frame centre's side of the horizon, and not on it).  A valid node gets P itself at r == 1, F itself at r == 0 and F + r (P - F)
otherwise; every other node keeps F bit for bit and counts in unfit[t].  residual[t] = the largest max(|Fx - Px| W0/2, |Fy - Py| H0/2) over the
valid nodes whose F is finite (0 without any): how far the field was from rigid, in source pixels."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_ref as HR  # noqa: E402
import zoom_ref as Z  # noqa: E402

FACTOR = Z.FACTOR        # the project's 4x rule
HORIZON = 2.0 ** -20     # a node is valid when D/Dc >= HORIZON
make_field = Z.make_field   # the identity grid plus a smooth perturbation plus 3 % noise

# the cases of tests/test_hip_rigid.py: the zoom kernel's shapes (the launch shape is the same) -- a partial wave, the smallest field, odd
# width and two column chunks
FRAME = Z.FRAME
SHAPES = Z.SHAPES
seed_of = Z.seed_of


def adjugate(M):
    """adj(M) of a (3, 3) matrix, the cofactors spelled out (no division), and det M from its first row."""
    m0, m1, m2, m3, m4, m5, m6, m7, m8 = (float(v) for v in np.asarray(M, np.float64).reshape(9))
    with np.errstate(all="ignore"):
        A = np.array([[m4 * m8 - m5 * m7, m2 * m7 - m1 * m8, m1 * m5 - m2 * m4],
                      [m5 * m6 - m3 * m8, m0 * m8 - m2 * m6, m2 * m3 - m0 * m5],
                      [m3 * m7 - m4 * m6, m1 * m6 - m0 * m7, m0 * m4 - m1 * m3]], np.float64)
        det = m0 * A[0, 0] + m1 * A[1, 0] + m2 * A[2, 0]
    return A, det


def node_uv(field_hw, frame_hw):
    """(u (fw,), v (fh,)) float64: the output positions the field's nodes stand for."""
    h0, w0 = frame_hw
    fh, fw = field_hw
    x, y = np.arange(fw, dtype=np.float64) * (w0 - 1) / (fw - 1), np.arange(fh, dtype=np.float64) * (h0 - 1) / (fh - 1)
    return 2 * x / w0 - 1, 2 * y / h0 - 1


def positions(M, field_hw, frame_hw):
    """(P64 (fh, fw, 2) float64, valid (fh, fw) bool, ratio (fh, fw) = D/Dc): a frame that is not fitted has no valid node."""
    A, det = adjugate(M)
    u, v = node_uv(field_hw, frame_hw)
    u, v = u[None, :], v[:, None]
    with np.errstate(all="ignore"):
        X, Y, D = (A[k, 0] * u + A[k, 1] * v + A[k, 2] for k in range(3))
        fitted = bool(np.isfinite(np.asarray(M, np.float64)).all() and np.isfinite(det) and det != 0 and A[2, 2] != 0)
        ratio = D / A[2, 2]
        valid = (ratio >= HORIZON) & fitted
        P = np.stack([X / D, Y / D], -1)
    return P, valid, ratio


def _stats(absdiff, valid, F, frame_hw):
    """max over the valid nodes with finite F of max(|dx| W0/2, |dy| H0/2), in absdiff's dtype; 0 without any."""
    h0, w0 = frame_hw
    half = np.array([w0 / 2, h0 / 2], absdiff.dtype)
    use = valid & np.isfinite(F).all(-1)
    d = (absdiff * half).max(-1)
    return d[use].max() if use.any() else absdiff.dtype.type(0)


def rigid64(field, m, frame_hw, r):
    """(out (T, fh, fw, 2) float64, residual (T,) float64, unfit (T,) int64): the definition in float64, P rounded to float32 as defined."""
    field = np.asarray(field, np.float32)
    T, fh, fw, _ = field.shape
    out = field.astype(np.float64)
    res, unfit = np.zeros(T), np.zeros(T, np.int64)
    for t in range(T):
        P, valid, _ = positions(np.asarray(m, np.float64).reshape(T, 9)[t], (fh, fw), frame_hw)
        with np.errstate(all="ignore"):
            P32 = P.astype(np.float32).astype(np.float64)
            F = out[t].copy()
            new = P32 if r == 1 else F if r == 0 else F + r * (P32 - F)
            out[t][valid] = new[valid]
            res[t] = _stats(np.abs(F - P32), valid, F, frame_hw)
        unfit[t] = int((~valid).sum())
    return out, res, unfit


def rigid32(field, m, frame_hw, r):
    """The kernel's operation sequence with the float32 part in numpy float32: P from float64 rounded once; the blend fma(r, P - F, F) (the
    compiler may contract F + r (P - F); Z._fma32 is zoom32's device for that); the residual |F - P| (one float32 subtraction) times the
    float32 W0/2 or H0/2.  (out float32, residual (T,) float32, unfit (T,) int64)."""
    field = np.asarray(field, np.float32)
    T, fh, fw, _ = field.shape
    out = field.copy()
    res, unfit = np.zeros(T, np.float32), np.zeros(T, np.int64)
    r32 = np.float32(r)
    for t in range(T):
        P, valid, _ = positions(np.asarray(m, np.float64).reshape(T, 9)[t], (fh, fw), frame_hw)
        with np.errstate(all="ignore"):
            P32 = P.astype(np.float32)
            F = field[t]
            new = P32 if r == 1 else F if r == 0 else Z._fma32(np.full(F.shape, r32, np.float32), (P32 - F).astype(np.float32), F)
            out[t][valid] = new[valid]
            res[t] = _stats(np.abs(F - P32).astype(np.float32), valid, F, frame_hw)
        unfit[t] = int((~valid).sum())
    return out, res, unfit


def coordinate_error_px(field, m, frame_hw):
    """The float32 sequence's own coordinate error, in source pixels: the largest difference, over every valid node with finite F, between
    its distance |F - P| (W0/2, H0/2) evaluated in float32 (as rigid32's residual is) and in float64; plus the share P's own float32
    rounding has in it, half an ulp of the largest |P| times max(W0, H0)/2."""
    field = np.asarray(field, np.float32)
    T, fh, fw, _ = field.shape
    h0, w0 = frame_hw
    worst = 0.0
    for t in range(T):
        P, valid, _ = positions(np.asarray(m, np.float64).reshape(T, 9)[t], (fh, fw), frame_hw)
        use = valid & np.isfinite(field[t]).all(-1)
        if not use.any():
            continue
        with np.errstate(all="ignore"):
            P32 = P.astype(np.float32)
            d32 = np.abs(field[t] - P32).astype(np.float32) * np.array([w0 / 2, h0 / 2], np.float32)
            d64 = np.abs(field[t].astype(np.float64) - P) * np.array([w0 / 2, h0 / 2])
        worst = max(worst, float(np.abs(d32.astype(np.float64) - d64)[use].max()))
    return worst


def make_homographies(n, seed):
    """(n, 9) float64, a different matrix per frame: the identity composed with a rotation of at most 2 degrees, a scale of 1 +- 3 %, a
    translation of at most 0.05 and perspective terms of at most 0.02, m33 = 1."""
    rs = np.random.RandomState(seed)
    out = np.empty((n, 9))
    for t in range(n):
        a, s = np.deg2rad(rs.uniform(-2, 2)), 1 + rs.uniform(-0.03, 0.03)
        tx, ty, p1, p2 = rs.uniform(-0.05, 0.05), rs.uniform(-0.05, 0.05), rs.uniform(-0.02, 0.02), rs.uniform(-0.02, 0.02)
        out[t] = [s * np.cos(a), -s * np.sin(a), tx, s * np.sin(a), s * np.cos(a), ty, p1, p2, 1.0]
    return out


def field_from_homography(H, field_hw, frame_hw):
    """(fh, fw, 2) float32: the exactly rigid field of H -- every node holds H^-1 of its output position -- through numpy's inverse, NOT
    through `positions`' adjugate, so that a test comparing the two compares two evaluations."""
    u, v = node_uv(field_hw, frame_hw)
    q = np.stack(np.broadcast_arrays(u[None, :], v[:, None], np.ones((len(v), len(u)))), -1) @ np.linalg.inv(np.asarray(H, np.float64).reshape(3, 3)).T
    return (q[..., :2] / q[..., 2:]).astype(np.float32)


def sample_lattice(field, frame_hw):
    """p1 (400, 2) float64 of one field (fh, fw, 2): the field resized to the frame (bilinear, align_corners=True) read at field_homography's
    20 x 20 lattice, in float64 (the kernel blends in float32)."""
    field = np.asarray(field, np.float64)
    fh, fw, _ = field.shape
    h0, w0 = frame_hw
    r, c, _ = HR.lattice(frame_hw)
    sy, sx = r * (fh - 1) / (h0 - 1), c * (fw - 1) / (w0 - 1)
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    y1, x1 = y0 + (y0 < fh - 1), x0 + (x0 < fw - 1)
    ly, lx = (sy - y0)[:, None], (sx - x0)[:, None]
    return (1 - ly) * ((1 - lx) * field[y0, x0] + lx * field[y0, x1]) + ly * ((1 - lx) * field[y1, x0] + lx * field[y1, x1])


def fit_field(field, frame_hw):
    """(M (3, 3), bounds (4,)) of one field through homography_ref: the fit pass 1 runs."""
    M = HR.fit(sample_lattice(field, frame_hw), HR.lattice(frame_hw)[2])
    return M, HR.bounds(M, frame_hw)


def refit_shift(fields, frame_hw):
    """The bounds rule, measured: every frame of ``fields`` is fitted, made fully rigid (rigid64, r = 1) and fitted again.  Returns (the largest
    difference of the four bounds, raw fit against refit, in source pixels; the largest |M_refit - M_raw| entry)."""
    px, dm = 0.0, 0.0
    for F in np.asarray(fields, np.float32):
        M, b = fit_field(F, frame_hw)
        out, _, unfit = rigid64(F[None], M.reshape(1, 9), frame_hw, 1.0)
        assert unfit[0] == 0
        M2, b2 = fit_field(out[0], frame_hw)
        px, dm = max(px, float(np.abs(b2 - b).max())), max(dm, float(np.abs(M2 - M).max()))
    return px, dm
