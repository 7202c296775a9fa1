"""numpy float64 restatement of rolling-shutter correction: the per-frame camera rates (csrc/path_smooth.hip pws_shutter_rates), the
row-dependent composition (csrc/field_compose.hip pws_field_compose_rows) and the analytic experiment that shows what the correction is
worth.  The affine composition, its tolerance terms, the fields and the path are tests/path_ref.py's.

Model.  motion[k] = (a, b, tx, ty) maps a point of frame k to frame k-1.  Row y (relative to the frame centre) of frame k was exposed at
time k + delta, delta = r clamp(y / (h0 - 1), -1/2, 1/2): r is the share of the frame interval that the readout from the top row to the
bottom row takes, negative for a sensor read bottom to top.  Between frames the camera moves at a constant velocity (l., w., x., y.) --
log scale, angle and translation per frame interval, in frame k's coordinates -- taken from motion[k+1] for delta >= 0 and from motion[k]
for delta < 0.  The position p0 of the global-shutter frame shows, in the rolling-shutter frame, at p = p0 - delta (l. p0 + w. J p0 +
(x., y.)), J p = (-p.y, p.x): first order in delta, with the row's time taken from p0."""
import math

import numpy as np

import path_ref as P


# ---------------------------------------------------------------------------------------------------------------- 1. rates

def _row(m):
    return tuple(float(v) for v in m) if np.isfinite(m).all() else (1.0, 0.0, 0.0, 0.0)


def forward_rate(m):
    """The velocity of frame k from motion[k+1], which maps frame k+1 into frame k: its generator, to first order."""
    a, b, tx, ty = _row(m)
    return (math.log(math.hypot(a, b)), math.atan2(b, a), tx, ty)


def backward_rate(m):
    """The velocity of frame k from motion[k], which maps frame k into frame k-1: the same generator seen from frame k."""
    a, b, tx, ty = _row(m)
    s, f = math.hypot(a, b), math.atan2(b, a)
    c, sn = math.cos(f), math.sin(f)
    return (math.log(s), f, (c * tx + sn * ty) / s, ((0.0 - sn) * tx + c * ty) / s)


def rates(motion):
    """One scene: (n, 2, 4) float64, [k, 0] the forward row, [k, 1] the backward row.  The first frame has no pair behind it and takes its
    forward row twice, the last frame its backward row; a scene of one frame stands still."""
    motion = np.asarray(motion, np.float64)
    n = motion.shape[0]
    out = np.zeros((n, 2, 4), np.float64)
    for k in range(n):
        fwd = forward_rate(motion[k + 1]) if k + 1 < n else None
        bwd = backward_rate(motion[k]) if k >= 1 else None
        if fwd is None and bwd is None:
            continue
        out[k, 0] = fwd if fwd is not None else bwd
        out[k, 1] = bwd if bwd is not None else fwd
    return out


def shutter_rates(motion, scene_cuts=None):
    """stream.shutter_rates: (T, 2, 4), scene by scene."""
    motion = np.asarray(motion, np.float64)
    T = motion.shape[0]
    edges = [0] + [int(c) for c in (scene_cuts or [])] + [T]
    out = np.zeros((T, 2, 4), np.float64)
    for a, b in zip(edges[:-1], edges[1:]):
        out[a:b] = rates(motion[a:b])
    return out


# ---------------------------------------------------------------------------------------------------------------- 2. composition

def positions64(d, rts, r, lattice, frame_hw):
    """p (T, fh, fw, 2): per node the position of the measured frame, in frame pixels relative to the centre, that the corrected frame
    shows there."""
    d, rts = np.asarray(d, np.float64), np.asarray(rts, np.float64)
    fh, fw = lattice
    h0, w0 = frame_hw
    kx, ky, cx, cy = (w0 - 1) / (fw - 1), (h0 - 1) / (fh - 1), 0.5 * (w0 - 1), 0.5 * (h0 - 1)
    y, x = np.meshgrid(np.arange(fh, dtype=np.float64) * ky - cy, np.arange(fw, dtype=np.float64) * kx - cx, indexing="ij")
    out = np.zeros((d.shape[0], fh, fw, 2), np.float64)
    ih = 1.0 / (h0 - 1)
    for t in range(d.shape[0]):
        with np.errstate(invalid="ignore", over="ignore"):
            p0x = d[t, 0] * x + d[t, 1] * y + d[t, 2]
            p0y = d[t, 3] * x + d[t, 4] * y + d[t, 5]
            delta = float(r) * np.clip(p0y * ih, -0.5, 0.5)
            v = np.where((delta >= 0)[..., None], rts[t, 0], rts[t, 1])
            out[t, ..., 0] = p0x - delta * (v[..., 0] * p0x - v[..., 1] * p0y + v[..., 2])
            out[t, ..., 1] = p0y - delta * (v[..., 0] * p0y + v[..., 1] * p0x + v[..., 3])
    return out


def copied(d_row, rts_row, r):
    """The frames the definition copies bit for bit."""
    return tuple(float(v) for v in d_row) == P.IDENTITY and (float(r) == 0.0 or not np.asarray(rts_row).any())


def compose_rows64(field, d, rts, r, frame_hw, return_terms=False):
    """The composed fields in float64 under the row-dependent correction; return_terms: also path_ref.compose64's two tolerance terms,
    evaluated at this function's own sample positions."""
    F = np.asarray(field, np.float64)
    T, fh, fw, _ = F.shape
    h0, w0 = frame_hw
    cx, cy, ikx, iky = 0.5 * (w0 - 1), 0.5 * (h0 - 1), (fw - 1) / (w0 - 1), (fh - 1) / (h0 - 1)
    p = positions64(d, rts, r, (fh, fw), frame_hw)
    out, tol = F.copy(), np.zeros_like(F)
    fmax = float(np.finfo(np.float32).max)
    for t in range(T):
        if copied(d[t], rts[t], r):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            sx, sy = (p[t, ..., 0] + cx) * ikx, (p[t, ..., 1] + cy) * iky
            ok = np.isfinite(sx) & np.isfinite(sy) & (np.abs(sx) <= fmax) & (np.abs(sy) <= fmax)
        sx, sy = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
        x0 = np.clip(np.floor(sx), 0, fw - 2).astype(np.int64)
        y0 = np.clip(np.floor(sy), 0, fh - 2).astype(np.int64)
        lx, ly = (sx - x0)[..., None], (sy - y0)[..., None]
        a, b, c, e = F[t][y0, x0], F[t][y0, x0 + 1], F[t][y0 + 1, x0], F[t][y0 + 1, x0 + 1]
        val = (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * e)
        out[t] = np.where(ok[..., None], val, F[t])
        corners = np.stack([a, b, c, e])
        W = (np.abs(1 - lx) + np.abs(lx)) * (np.abs(1 - ly) + np.abs(ly))
        tol[t] = np.where(ok[..., None], 2.0 ** -22 * W * np.abs(corners).max(0) + 2.0 ** -16 * (corners.max(0) - corners.min(0)), 0.0)
    return (out, tol) if return_terms else out


def identity_field(T, lattice):
    fh, fw = lattice
    u, v = np.meshgrid(np.linspace(-1, 1, fw), np.linspace(-1, 1, fh))
    return np.stack([np.stack([u, v], -1)] * T).astype(np.float32)


def field_positions(composed, frame_hw):
    """A composed IDENTITY field read as positions: p(q) in frame pixels relative to the centre."""
    h0, w0 = frame_hw
    c = np.asarray(composed, np.float64)
    return np.stack([c[..., 0] * (0.5 * (w0 - 1)), c[..., 1] * (0.5 * (h0 - 1))], -1)


# ---------------------------------------------------------------------------------------------------------------- 3. the experiment
# A camera whose pose is known at every instant: frame pixel p exposed at time tau shows the world at Rot(theta(tau)) p + T(tau)
# (motion_ref.texture_clip's convention).  The path is a pan plus a few slow sinusoids: hand shake of 1 to 3 pixels and 0.2 degree with
# periods of 11 to 29 frames, which a linear path between frames follows.

N, SIZE, R_TRUE, SIGMA, LATTICE = 32, 256, 0.8, 4.0, (33, 33)
PAN = (1.5, 0.5)
SHAKE_X = ((3.0, 13.0, 0.3), (1.5, 29.0, 1.1))     # (amplitude [px], period [frames], phase)
SHAKE_Y = ((2.5, 17.0, 2.0), (1.0, 11.0, 0.4))
SHAKE_TH = ((0.2, 19.0, 0.7),)                     # amplitude in degrees


def pose(tau):
    """(theta [rad], tx, ty) at time tau (any array shape)."""
    tau = np.asarray(tau, np.float64)
    tx, ty, th = PAN[0] * tau, PAN[1] * tau, np.zeros_like(tau)
    for a, per, ph in SHAKE_X:
        tx = tx + a * np.sin(2 * np.pi * tau / per + ph)
    for a, per, ph in SHAKE_Y:
        ty = ty + a * np.sin(2 * np.pi * tau / per + ph)
    for a, per, ph in SHAKE_TH:
        th = th + np.deg2rad(a) * np.sin(2 * np.pi * tau / per + ph)
    return th, tx, ty


def analytic_motion(n=N):
    """motion (n, 4) between the poses at the frames' centre rows (motion_ref.expected_motion, as (a, b, tx, ty))."""
    th, tx, ty = pose(np.arange(n, dtype=np.float64))
    m = np.zeros((n, 4), np.float64)
    m[0] = (1.0, 0.0, 0.0, 0.0)
    for k in range(1, n):
        dth, dx, dy = th[k] - th[k - 1], tx[k] - tx[k - 1], ty[k] - ty[k - 1]
        c, s = math.cos(th[k - 1]), math.sin(th[k - 1])
        m[k] = (math.cos(dth), math.sin(dth), c * dx + s * dy, -s * dx + c * dy)
    return m


def non_rigidity(p, frame_hw, r_true=R_TRUE):
    """p (T, fh, fw, 2): the position of rolling-shutter frame k that output node q of frame k shows.  That pixel lies on a row exposed at
    tau = k + r_true clamp(p.y / (h0 - 1), -1/2, 1/2) and shows the world at X = pose(tau) p.  A rigid output frame has q -> X a
    similarity; per frame the best one is fitted by least squares.  Returns the RMS residual over all nodes and frames, in pixels (the
    poses keep the scale at 1)."""
    T, fh, fw, _ = p.shape
    h0, w0 = frame_hw
    kx, ky, cx, cy = (w0 - 1) / (fw - 1), (h0 - 1) / (fh - 1), 0.5 * (w0 - 1), 0.5 * (h0 - 1)
    qy, qx = np.meshgrid(np.arange(fh, dtype=np.float64) * ky - cy, np.arange(fw, dtype=np.float64) * kx - cx, indexing="ij")
    qx, qy = qx.ravel(), qy.ravel()
    total = 0.0
    for k in range(T):
        px, py = p[k, ..., 0].ravel(), p[k, ..., 1].ravel()
        th, tx, ty = pose(k + r_true * np.clip(py / (h0 - 1), -0.5, 0.5))
        X, Y = np.cos(th) * px - np.sin(th) * py + tx, np.sin(th) * px + np.cos(th) * py + ty
        # X = a qx - b qy + e, Y = b qx + a qy + f
        A = np.zeros((2 * qx.size, 4), np.float64)
        A[0::2, 0], A[0::2, 1], A[0::2, 2] = qx, -qy, 1.0
        A[1::2, 0], A[1::2, 1], A[1::2, 3] = qy, qx, 1.0
        rhs = np.empty(2 * qx.size, np.float64)
        rhs[0::2], rhs[1::2] = X, Y
        sol = np.linalg.lstsq(A, rhs, rcond=None)[0]
        res = A @ sol - rhs
        total += float((res[0::2] ** 2 + res[1::2] ** 2).mean())
    return math.sqrt(total / T)


def experiment(compose=None, motion=None, n=N, sigma=SIGMA):
    """(e(+r), e(0), e(-r)): the non-rigidity of the output under smoothing with the correction, without it and with the wrong sign.
    ``compose(field, d, rates, r)`` returns the composed field (default: compose_rows64); ``motion`` defaults to the analytic one."""
    hw = (SIZE, SIZE)
    motion = analytic_motion(n) if motion is None else motion
    _, d = P.path_smooth(motion, sigma)
    rts = rates(motion)
    field = identity_field(n, LATTICE)
    compose = compose or (lambda f, dd, rr, r: compose_rows64(f, dd, rr, r, hw))
    return tuple(non_rigidity(field_positions(compose(field, d, rts, r), hw), hw) for r in (R_TRUE, 0.0, -R_TRUE))
