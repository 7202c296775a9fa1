"""numpy float64 restatement of the rolling-shutter estimate (csrc/shutter_estimate.hip pws_shutter_terms / pws_shutter_estimate;
stream.estimate_rolling_shutter) and the analytic rolling-shutter clips that show what it recovers.  The block search, the validity rule,
the sub-pixel vectors and the summation orders are tests/motion_ref.py's, the rates and the analytic camera tests/shutter_ref.py's.

Model.  Row y (relative to the centre) of frame k is exposed at k + r c, c = clamp(y / (H0 - 1), -1/2, 1/2).  A block of frame k on that row
is found in frame k-1 on (nearly) the same row, exposed at k - 1 + r c: between the two exposures the camera moved by the pair's motion plus
r c times the change of its velocity from one frame interval to the next.  A similarity absorbs the first; the second, z = c (dl p + dw J p +
(dx, dy)) with dV = rates[k] - rates[k-1], it cannot.  r is the one coefficient of z, after both the vectors and z have had their own
least-squares similarity taken out, shared by every pair of the clip."""
import math

import numpy as np

import motion_ref as R
import shutter_ref as S

MIN_BLOCKS = R.MIN_BLOCKS


# ---------------------------------------------------------------------------------------------------------------- 1. the definition

def valid_blocks(mv, sad, act, h, w, radius, min_activity, scale):
    """[(x, y, dx, dy)] of one pair's blocks that pass the fit's validity rule, centres and sub-pixel vectors times (sx, sy)."""
    Rr = int(radius)
    sx_, sy_ = float(scale[0]), float(scale[1])
    nby, nbx = mv.shape[:2]
    cx0, cy0 = 0.5 * (w - 1), 0.5 * (h - 1)
    blocks = []
    for i in range(nby * nbx):
        by, bx = divmod(i, nbx)
        dxi, dyi = int(mv[by, bx, 0]), int(mv[by, bx, 1])
        if act[by, bx] < min_activity or abs(dxi) >= Rr or abs(dyi) >= Rr:
            continue
        s = [int(v) for v in sad[by, bx]]
        if 2 * ((s[1] - 2 * s[0] + s[2]) + (s[3] - 2 * s[0] + s[4])) < int(act[by, bx]):
            continue
        ox, oy = R.subpixel(sad[by, bx])
        blocks.append((((Rr + R.B * bx + 7.5) - cx0) * sx_, ((Rr + R.B * by + 7.5) - cy0) * sy_, (dxi + ox) * sx_, (dyi + oy) * sy_))
    return blocks


def _res2(f, b):
    a1, bb, tx, ty = f
    x, y, dx, dy = b
    rx, ry = ((a1 * x - bb * y) + tx) - dx, ((bb * x + a1 * y) + ty) - dy
    return rx * rx + ry * ry


def _similarity(s0, sx, sy, den, sdx, sdy, c, d):
    """The fit's closed-form normal equations: (a - 1, b, tx, ty) from the sums."""
    a1 = (c - (sx * sdx + sy * sdy) / s0) / den
    bb = (d - (sx * sdy - sy * sdx) / s0) / den
    return a1, bb, ((sdx - a1 * sx) + bb * sy) / s0, ((sdy - bb * sx) - a1 * sy) / s0


ZERO = (0.0, 0.0, 0.0, 0.0)


def pair_terms(mv, sad, act, m, dv, h, w, radius, min_activity=2000, scale=(1.0, 1.0), h0=None, order="forward", margins=None):
    """One usable pair's (sum e . z_perp, sum z_perp . z_perp, sum e . e, count).  m: the pair's returned motion (a, b, tx, ty); dv (2, 4):
    rates[k] - rates[k-1], forward and backward.  margins (a list): gets per valid block the relative distance of its squared residual from
    the inlier threshold."""
    sx_, sy_ = float(scale[0]), float(scale[1])
    h0 = float(h) if h0 is None else float(h0)
    blocks = valid_blocks(mv, sad, act, h, w, radius, min_activity, scale)
    if len(blocks) < MIN_BLOCKS:
        return ZERO
    f = (float(m[0]) - 1.0, float(m[1]), float(m[2]), float(m[3]))
    r2 = [_res2(f, b) for b in blocks]
    thr = max(sx_ * sy_, 4.0 * (R._sum(r2, order) / float(len(blocks))))
    if margins is not None:
        margins.extend(abs(v - thr) / thr for v in r2)
    kept = [b for b, v in zip(blocks, r2) if v <= thr]
    n = len(kept)
    if n < MIN_BLOCKS:
        return ZERO
    z = []
    for x, y, _, _ in kept:
        c = min(0.5, max(-0.5, y / (h0 - 1.0)))
        dl, dw, dx, dy = (float(v) for v in (dv[0] if c >= 0.0 else dv[1]))
        z.append((c * ((dl * x - dw * y) + dx), c * ((dl * y + dw * x) + dy)))
    s0 = float(n)
    sx, sy = R._sum((b[0] for b in kept), order), R._sum((b[1] for b in kept), order)
    sq = R._sum((b[0] * b[0] + b[1] * b[1] for b in kept), order)
    den = sq - (sx * sx + sy * sy) / s0
    if not den > 0.0:
        return ZERO
    fv = _similarity(s0, sx, sy, den, R._sum((b[2] for b in kept), order), R._sum((b[3] for b in kept), order),
                     R._sum((b[0] * b[2] + b[1] * b[3] for b in kept), order), R._sum((b[0] * b[3] - b[1] * b[2] for b in kept), order))
    fz = _similarity(s0, sx, sy, den, R._sum((q[0] for q in z), order), R._sum((q[1] for q in z), order),
                     R._sum((b[0] * q[0] + b[1] * q[1] for b, q in zip(kept, z)), order),
                     R._sum((b[0] * q[1] - b[1] * q[0] for b, q in zip(kept, z)), order))

    def resid(fit, x, y, ux, uy):
        return ux - ((fit[0] * x - fit[1] * y) + fit[2]), uy - ((fit[1] * x + fit[0] * y) + fit[3])
    e = [resid(fv, b[0], b[1], b[2], b[3]) for b in kept]
    zp = [resid(fz, b[0], b[1], q[0], q[1]) for b, q in zip(kept, z)]
    return (R._sum((a[0] * q[0] + a[1] * q[1] for a, q in zip(e, zp)), order), R._sum((q[0] * q[0] + q[1] * q[1] for q in zp), order),
            R._sum((a[0] * a[0] + a[1] * a[1] for a in e), order), s0)


def usable_pairs(motion, scene_cuts=None):
    """Pair k of a scene [a, b) is usable when a + 2 <= k <= b - 2 and rows k-1, k, k+1 of ``motion`` are finite: both velocity differences
    then come from real pairs, never from a scene end's duplicated rate."""
    motion = np.asarray(motion, np.float64)
    T = motion.shape[0]
    edges = [0] + [int(c) for c in (scene_cuts or [])] + [T]
    ok = np.zeros(T, bool)
    for a, b in zip(edges[:-1], edges[1:]):
        for k in range(a + 2, b - 1):
            ok[k] = bool(np.isfinite(motion[k - 1:k + 2]).all())
    return ok


def terms(mv, sad, act, motion, rates, h, w, radius=16, min_activity=2000, scale=(1.0, 1.0), h0=None, scene_cuts=None, order="forward",
          margins=None):
    """(T, 4) float64: a row per pair, zero for every pair that is not usable or keeps fewer than 8 blocks."""
    motion, rates = np.asarray(motion, np.float64), np.asarray(rates, np.float64)
    T = motion.shape[0]
    out = np.zeros((T, 4), np.float64)
    for k in np.flatnonzero(usable_pairs(motion, scene_cuts)):
        out[k] = pair_terms(mv[k], sad[k], act[k], motion[k], rates[k] - rates[k - 1], h, w, radius, min_activity, scale, h0, order, margins)
    return out


def estimate(tm, order="forward"):
    """(r_hat, se, D, n) from the terms' column sums over all rows; (NaN, inf, D, n) when D or the degrees of freedom are not positive."""
    tm = np.asarray(tm, np.float64).reshape(-1, 4)
    N, D, E, n = (R._sum(tm[:, c], order) for c in range(4))
    m = int((tm[:, 3] > 0).sum())
    dof = 2.0 * n - 4.0 * m - 1.0
    if not (D > 0.0 and dof > 0.0):
        return np.array([math.nan, math.inf, D, n], np.float64)
    r = N / D
    return np.array([r, math.sqrt(max(0.0, E - r * N) / dof / D), D, n], np.float64)


def estimate_clip(planes, radius=16, min_activity=2000, scene_cuts=None, order="forward", return_terms=False):
    """Planes to estimate, all in the restatements: block search, fit, rates under the cuts, terms, estimate (plane pixels)."""
    planes = np.asarray(planes, np.float32)
    h, w = planes.shape[1:]
    mv, sad, act = R.block_motion(planes, radius)
    motion, _ = R.motion_fit(mv, sad, act, h, w, radius, min_activity)
    tm = terms(mv, sad, act, motion, S.shutter_rates(motion, scene_cuts), h, w, radius, min_activity, scene_cuts=scene_cuts, order=order)
    est = estimate(tm, order)
    return (est, tm, motion, (mv, sad, act)) if return_terms else est


def choose(est, max_se=0.02):
    """What VideoStabilizer(rolling_shutter="auto") uses: clamp(r_hat, -1, 1) when r_hat is finite and se <= max_se, else 0.0."""
    r, se = float(est[0]), float(est[1])
    return min(1.0, max(-1.0, r)) if math.isfinite(r) and se <= max_se else 0.0


# ---------------------------------------------------------------------------------------------------------------- 2. rolling-shutter clips
# shutter_ref's camera plus two faster components: hand shake has them, and the estimate lives on acceleration.

FAST_X = ((1.0, 5.3, 0.9),)    # (amplitude [px], period [frames], phase)
FAST_Y = ((0.8, 6.1, 2.2),)


def pose(tau, fast=True, gain=1.0):
    """(theta, tx, ty) at time tau: shutter_ref.pose, the two faster components added, the shake (not the pan) times ``gain``."""
    tau = np.asarray(tau, np.float64)
    th, tx, ty = S.pose(tau)
    if fast:
        for a, per, ph in FAST_X:
            tx = tx + a * np.sin(2 * np.pi * tau / per + ph)
        for a, per, ph in FAST_Y:
            ty = ty + a * np.sin(2 * np.pi * tau / per + ph)
    if gain != 1.0:
        px, py = S.PAN[0] * tau, S.PAN[1] * tau
        th, tx, ty = gain * th, px + gain * (tx - px), py + gain * (ty - py)
    return th, tx, ty


def pan_pose(tau):
    """A steady pan, no shake: a clip without information about r."""
    tau = np.asarray(tau, np.float64)
    return np.zeros_like(tau), S.PAN[0] * tau, S.PAN[1] * tau


def rolling_clip(r, n=S.N, h=S.SIZE, w=S.SIZE, seed=7, pose_fn=pose):
    """motion_ref.texture_clip's texture under a rolling shutter: row y (relative to the centre) of frame t is exposed at
    t + r clamp(y / (h - 1), -1/2, 1/2) and shows the texture under the pose of that instant, evaluated there: nothing is resampled."""
    rs = np.random.RandomState(seed)
    lam = rs.uniform(5.0, 48.0, 24)
    ang = rs.uniform(0.0, 2 * np.pi, 24)
    ph = rs.uniform(0.0, 2 * np.pi, 24)
    kx, ky = 2 * np.pi / lam * np.cos(ang), 2 * np.pi / lam * np.sin(ang)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64) - 0.5 * (h - 1), np.arange(w, dtype=np.float64) - 0.5 * (w - 1), indexing="ij")
    delta = float(r) * np.clip(yy / (h - 1), -0.5, 0.5)
    out = np.empty((n, h, w), np.float32)
    for t in range(n):
        th, tx, ty = pose_fn(t + delta)
        X = np.cos(th) * xx - np.sin(th) * yy + tx
        Y = np.sin(th) * xx + np.cos(th) * yy + ty
        v = np.zeros((h, w), np.float64)
        for i in range(24):
            v += np.sin(kx[i] * X + ky[i] * Y + ph[i])
        out[t] = (0.11 * v).astype(np.float32)
    return out


def non_rigidity(p, frame_hw, r_true, pose_fn=pose):
    """shutter_ref.non_rigidity under this file's camera: output node q of frame k shows position p of the rolling-shutter frame, exposed at
    k + r_true clamp(p.y / (h0 - 1), -1/2, 1/2), hence the world at X = pose(tau) p; the RMS residual of q -> X against the best similarity per
    frame, in pixels."""
    T, fh, fw, _ = p.shape
    h0, w0 = frame_hw
    qy, qx = np.meshgrid(np.arange(fh, dtype=np.float64) * ((h0 - 1) / (fh - 1)) - 0.5 * (h0 - 1),
                         np.arange(fw, dtype=np.float64) * ((w0 - 1) / (fw - 1)) - 0.5 * (w0 - 1), indexing="ij")
    qx, qy = qx.ravel(), qy.ravel()
    A = np.zeros((2 * qx.size, 4), np.float64)   # X = a qx - b qy + e, Y = b qx + a qy + f
    A[0::2, 0], A[0::2, 1], A[0::2, 2] = qx, -qy, 1.0
    A[1::2, 0], A[1::2, 1], A[1::2, 3] = qy, qx, 1.0
    total = 0.0
    for k in range(T):
        px, py = p[k, ..., 0].ravel(), p[k, ..., 1].ravel()
        th, tx, ty = pose_fn(k + r_true * np.clip(py / (h0 - 1), -0.5, 0.5))
        rhs = np.empty(2 * qx.size, np.float64)
        rhs[0::2], rhs[1::2] = np.cos(th) * px - np.sin(th) * py + tx, np.sin(th) * px + np.cos(th) * py + ty
        res = A @ np.linalg.lstsq(A, rhs, rcond=None)[0] - rhs
        total += float((res[0::2] ** 2 + res[1::2] ** 2).mean())
    return math.sqrt(total / T)


def end_to_end(motion, r_used, r_true, sigma=S.SIGMA, pose_fn=pose):
    """The non-rigidity of the output when a clip exposed under r_true, with this measured motion, is smoothed and corrected with r_used."""
    import path_ref as P
    hw = (S.SIZE, S.SIZE)
    _, d = P.path_smooth(motion, sigma)
    field = S.identity_field(motion.shape[0], S.LATTICE)
    composed = S.compose_rows64(field, d, S.rates(motion), r_used, hw)
    return non_rigidity(S.field_positions(composed, hw), hw, r_true, pose_fn)
