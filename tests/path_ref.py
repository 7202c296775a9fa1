"""numpy float64 restatement of path smoothing: the motion fit in frame pixels (csrc/motion.hip pws_motion_fit_scaled), the camera path, its
Gaussian low-pass and the corrections (csrc/path_smooth.hip) and the composition of a correction into a warp field (csrc/field_compose.hip).
The block search, the sub-pixel rule, the summation orders and the synthetic clips are tests/motion_ref.py's."""
import math

import numpy as np

import motion_ref as R

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------- 1. the scaled fit

def fit_pair_scaled(mv, sad, act, h, w, radius, min_activity=2000, scale=(1.0, 1.0), order="forward", margins=None):
    """motion_ref.fit_pair with every block centre and sub-pixel vector multiplied by (sx, sy) before the sums, and the outlier floor
    sx * sy in place of 1.0.  At (1, 1) every product is exact: motion_ref.fit_pair's bits."""
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
    nan = (math.nan,) * 4

    def res2(f, b):
        a1, bb, tx, ty = f
        x, y, dx, dy = b
        rx, ry = ((a1 * x - bb * y) + tx) - dx, ((bb * x + a1 * y) + ty) - dy
        return rx * rx + ry * ry
    used, fit = blocks, None
    for rnd in range(3):
        if rnd > 0:
            r2 = [res2(fit, b) for b in blocks]
            if margins is not None:
                margins.extend(abs(v - thr) / thr for v in r2)
            used = [b for b, v in zip(blocks, r2) if v <= thr]
        n = len(used)
        if n < R.MIN_BLOCKS:
            return nan, 0
        s0 = float(n)
        sx, sy = R._sum((b[0] for b in used), order), R._sum((b[1] for b in used), order)
        sq = R._sum((b[0] * b[0] + b[1] * b[1] for b in used), order)
        sdx, sdy = R._sum((b[2] for b in used), order), R._sum((b[3] for b in used), order)
        c = R._sum((b[0] * b[2] + b[1] * b[3] for b in used), order)
        d = R._sum((b[0] * b[3] - b[1] * b[2] for b in used), order)
        den = sq - (sx * sx + sy * sy) / s0
        if not den > 0.0:
            return nan, 0
        a1 = (c - (sx * sdx + sy * sdy) / s0) / den
        bb = (d - (sx * sdy - sy * sdx) / s0) / den
        tx = ((sdx - a1 * sx) + bb * sy) / s0
        ty = ((sdy - bb * sx) - a1 * sy) / s0
        fit = (a1, bb, tx, ty)
        if rnd < 2:
            thr = max(sx_ * sy_, 4.0 * (R._sum((res2(fit, b) for b in used), order) / s0))
    return (1.0 + fit[0], fit[1], fit[2], fit[3]), n


def motion_fit_scaled(mv, sad, act, h, w, radius=16, min_activity=2000, scale=(1.0, 1.0), order="forward", margins=None):
    """motion (n, 4) float64 in frame pixels and inliers (n,) int32; row 0 is (1, 0, 0, 0) with 0 inliers."""
    n = mv.shape[0]
    motion = np.zeros((n, 4), np.float64)
    inl = np.zeros((n,), np.int32)
    for t in range(n):
        if t == 0:
            motion[0] = (1.0, 0.0, 0.0, 0.0)
            continue
        motion[t], inl[t] = fit_pair_scaled(mv[t], sad[t], act[t], h, w, radius, min_activity, scale, order, margins)
    return motion, inl


def global_motion_scaled(planes, scale, radius=16, min_activity=2000):
    planes = np.asarray(planes, np.float32)
    mv, sad, act = R.block_motion(planes, radius)
    return motion_fit_scaled(mv, sad, act, planes.shape[1], planes.shape[2], radius, min_activity, scale)


# ---------------------------------------------------------------------------------------------------------------- 2. path and corrections

def camera_path(motion):
    """P (n, 4) = (lambda, theta, cx, cy): the pose of frame k in frame 0's coordinates.  Row 0 of ``motion`` is not read; a row with an
    entry that is not finite counts as (1, 0, 0, 0)."""
    motion = np.asarray(motion, np.float64)
    n = motion.shape[0]
    P = np.zeros((n, 4), np.float64)
    lam = th = cx = cy = 0.0
    for k in range(1, n):
        a, b, tx, ty = (float(v) for v in motion[k]) if np.isfinite(motion[k]).all() else (1.0, 0.0, 0.0, 0.0)
        s, c, sn = math.exp(lam), math.cos(th), math.sin(th)
        cx, cy = cx + s * (c * tx - sn * ty), cy + s * (sn * tx + c * ty)
        lam = lam + math.log(math.hypot(a, b))
        th = th + math.atan2(b, a)
        P[k] = (lam, th, cx, cy)
    return P


def smooth(P, sigma):
    """The normalised Gaussian average over k - Re .. k + Re, Re = min(ceil(3 sigma), n - 1), summed in ascending offset; beyond the ends P is
    continued by odd reflection."""
    n = P.shape[0]
    Re = min(int(math.ceil(3.0 * sigma)), n - 1)
    g = [math.exp(-0.5 * ((k / sigma) * (k / sigma))) for k in range(Re + 1)]

    def at(j):
        if j < 0:
            return 2.0 * P[0] - P[-j]
        if j > n - 1:
            return 2.0 * P[n - 1] - P[2 * (n - 1) - j]
        return P[j]
    out = np.zeros_like(P)
    for k in range(n):
        acc, ws = np.zeros(4, np.float64), 0.0
        for dl in range(-Re, Re + 1):
            acc = acc + g[abs(dl)] * at(k + dl)
            ws = ws + g[abs(dl)]
        out[k] = acc / ws
    return out


def corrections(P, Ph):
    """D (n, 6), row-major 2 x 3: C_k^-1 o C^_k."""
    D = np.zeros((P.shape[0], 6), np.float64)
    for k in range(P.shape[0]):
        lam, th, cx, cy = (float(v) for v in P[k])
        dlam, dth, ux, uy = (float(v) for v in Ph[k] - P[k])
        s, e, c, sn = math.exp(dlam), math.exp(-lam), math.cos(th), math.sin(th)
        D[k] = (s * math.cos(dth), 0.0 - s * math.sin(dth), e * (c * ux + sn * uy), s * math.sin(dth), s * math.cos(dth), e * (c * uy - sn * ux))
    return D


def path_smooth(motion, sigma):
    """One scene: (path (n, 4), D (n, 6))."""
    P = camera_path(motion)
    return P, corrections(P, smooth(P, float(sigma)))


def smooth_path(motion, sigma, scene_cuts=None):
    """stream.smooth_path: (D (T, 6), path (T, 4)), scene by scene."""
    motion = np.asarray(motion, np.float64)
    T = motion.shape[0]
    edges = [0] + [int(c) for c in (scene_cuts or [])] + [T]
    D, P = np.zeros((T, 6), np.float64), np.zeros((T, 4), np.float64)
    for a, b in zip(edges[:-1], edges[1:]):
        P[a:b], D[a:b] = path_smooth(motion[a:b], sigma)
    return D, P


# ---------------------------------------------------------------------------------------------------------------- 3. composition

def compose64(field, d, frame_hw, return_terms=False):
    """The composed fields in float64: field (T, fh, fw, 2), d (T, 6) float64.  return_terms: also, per value, the float32 kernel's allowed
    distance -- 2^-22 W max|corner| (three roundings of the blend under the weights' absolute sum W = (|1 - lx| + |lx|)(|1 - ly| + |ly|)) plus
    2^-16 max|corner difference| (one float32 rounding of each lattice coordinate, which is at most 256)."""
    F = np.asarray(field, np.float64)
    d = np.asarray(d, np.float64)
    T, fh, fw, _ = F.shape
    h0, w0 = frame_hw
    kx, ky, cx, cy = (w0 - 1) / (fw - 1), (h0 - 1) / (fh - 1), 0.5 * (w0 - 1), 0.5 * (h0 - 1)
    ikx, iky = (fw - 1) / (w0 - 1), (fh - 1) / (h0 - 1)
    out, tol = F.copy(), np.zeros_like(F)
    y, x = np.meshgrid(np.arange(fh, dtype=np.float64) * ky - cy, np.arange(fw, dtype=np.float64) * kx - cx, indexing="ij")
    fmax = float(np.finfo(np.float32).max)
    for t in range(T):
        if tuple(float(v) for v in d[t]) == IDENTITY:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            sx = ((d[t, 0] * x + d[t, 1] * y + d[t, 2]) + cx) * ikx
            sy = ((d[t, 3] * x + d[t, 4] * y + d[t, 5]) + cy) * iky
            ok = np.isfinite(sx) & np.isfinite(sy) & (np.abs(sx) <= fmax) & (np.abs(sy) <= fmax)   # (beyond float32: infinite once rounded)
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


def unnormalize64(g, size, align_corners):
    g = np.asarray(g, np.float64)
    return (g + 1) / 2 * (size - 1) if align_corners else ((g + 1) * size - 1) / 2


def uncovered_bounds(out64, tol, frame_hw, align_corners, m):
    """Per frame (lo, hi, undecided share): a node is covered iff m <= ix <= W0-1-m and m <= iy <= H0-1-m (NaN: not covered).  A node whose
    coordinate lies within the value tolerance -- in pixels: tol * size / 2, plus one float32 rounding of the un-normalised coordinate -- of a
    threshold is undecided; the kernel's count lies in [lo, lo + undecided]."""
    h0, w0 = frame_hw
    ix, iy = unnormalize64(out64[..., 0], w0, align_corners), unnormalize64(out64[..., 1], h0, align_corners)
    dx = tol[..., 0] * (0.5 * w0) + float(np.spacing(np.float32(w0)))
    dy = tol[..., 1] * (0.5 * h0) + float(np.spacing(np.float32(h0)))
    with np.errstate(invalid="ignore"):
        cov = (ix >= m) & (ix <= w0 - 1 - m) & (iy >= m) & (iy <= h0 - 1 - m)
        near = (np.minimum(np.abs(ix - m), np.abs(ix - (w0 - 1 - m))) <= dx) | (np.minimum(np.abs(iy - m), np.abs(iy - (h0 - 1 - m))) <= dy)
    near = near & ~(np.isnan(ix) | np.isnan(iy))
    n = cov.shape[0]
    lo = (~cov & ~near).reshape(n, -1).sum(1)
    return lo, lo + near.reshape(n, -1).sum(1), float(near.mean())


def make_field(shape, seed, scale=1.0, amp=0.05):
    """(T, fh, fw, 2) float32: the identity grid in [-1, 1] x ``scale`` plus a smooth random perturbation (no noise: a field is smooth)."""
    T, fh, fw, _ = shape
    rs = np.random.RandomState(seed)
    u, v = np.meshgrid(np.linspace(-1, 1, fw), np.linspace(-1, 1, fh))
    out = np.empty(shape, np.float64)
    for t in range(T):
        p = rs.uniform(0, 2 * np.pi, 4)
        out[t, ..., 0] = scale * u + amp * np.sin(np.pi * u + p[0]) * np.cos(0.5 * np.pi * v + p[1])
        out[t, ..., 1] = scale * v + amp * np.cos(np.pi * v + p[2]) * np.sin(0.7 * np.pi * u + p[3])
    return out.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the experiment

def texture_affine(poses, corr, h, w, seed):
    """motion_ref.texture_clip seen through per-frame corrections: pixel p (relative to the plane centre) of output frame t shows the source
    frame at q = D_t p, i.e. the texture at Rot(theta_t) q + T_t, evaluated there -- nothing is resampled.  The sinusoids are
    texture_clip's (same seed, same draws)."""
    rs = np.random.RandomState(seed)
    lam = rs.uniform(5.0, 48.0, 24)
    ang = rs.uniform(0.0, 2 * np.pi, 24)
    ph = rs.uniform(0.0, 2 * np.pi, 24)
    kx, ky = 2 * np.pi / lam * np.cos(ang), 2 * np.pi / lam * np.sin(ang)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64) - 0.5 * (h - 1), np.arange(w, dtype=np.float64) - 0.5 * (w - 1), indexing="ij")
    out = np.empty((len(poses), h, w), np.float32)
    for t, (th, tx, ty) in enumerate(poses):
        d = corr[t]
        qx, qy = d[0] * xx + d[1] * yy + d[2], d[3] * xx + d[4] * yy + d[5]
        X = math.cos(th) * qx - math.sin(th) * qy + tx
        Y = math.sin(th) * qx + math.cos(th) * qy + ty
        v = np.zeros((h, w), np.float64)
        for i in range(24):
            v += np.sin(kx[i] * X + ky[i] * Y + ph[i])
        out[t] = (0.11 * v).astype(np.float32)
    return out


def experiment(n=48, path_seed=5, clip_seed=7, sigma=4.0, size=256):
    """(stability in, stability out): a shaky analytic clip measured, its path smoothed, the clip rendered again through the corrections and
    measured again."""
    poses = R.planted_path(n, seed=path_seed)
    clip = R.texture_clip(poses, size, size, seed=clip_seed)
    motion, _ = R.global_motion(clip)
    s_in = R.stability_scores(motion)["stability"]
    _, D = path_smooth(motion, sigma)
    motion_out, _ = R.global_motion(texture_affine(poses, D, size, size, clip_seed))
    return s_in, R.stability_scores(motion_out)["stability"]
