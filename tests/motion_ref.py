"""numpy restatement of the global-motion measurement (csrc/motion.hip, stream.block_motion / global_motion / stability_scores): the
quantisation in float32, one rounding per step; the SADs, the tie rule and the activity in integers; the similarity fit and the stability
scores in float64.  The fit's sums can be taken in three orders, which is how the GPU test measures its tolerance."""
import math

import numpy as np

B = 16            # block side
MIN_BLOCKS = 8    # fewer blocks in any round of the fit: a NaN row


def quant(v):
    """q = min(255, max(0, floor((v + 1) * 127.5 + 0.5))), 0 for NaN; float32, every step rounded once."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = (v + np.float32(1)) * np.float32(127.5) + np.float32(0.5)
        assert c.dtype == np.float32
        c = np.where(np.isnan(c), np.float32(0), c)
        return np.floor(np.clip(c, np.float32(0), np.float32(255))).astype(np.uint8)


def lattice(h, w, radius):
    return (h - 2 * radius) // B, (w - 2 * radius) // B


def candidates(radius):
    """[(dy, dx)] in raster order, and each one's rank in the order sorted by (dx^2 + dy^2, dy, dx)."""
    cand = [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]
    order = sorted(range(len(cand)), key=lambda i: (cand[i][0] ** 2 + cand[i][1] ** 2, cand[i][0], cand[i][1]))
    rank = np.empty(len(cand), np.int64)
    rank[order] = np.arange(len(cand))
    return cand, rank


def activity_of(q, radius):
    """(nby, nbx) int32: sum over each block of |q[y, x+1] - q[y, x]| (16 x 15 pairs) + |q[y+1, x] - q[y, x]| (15 x 16 pairs)."""
    h, w = q.shape
    nby, nbx = lattice(h, w, radius)
    blocks = q[radius:radius + B * nby, radius:radius + B * nbx].astype(np.int32).reshape(nby, B, nbx, B).transpose(0, 2, 1, 3)
    return (np.abs(np.diff(blocks, axis=3)).sum((2, 3)) + np.abs(np.diff(blocks, axis=2)).sum((2, 3))).astype(np.int32)


def block_motion(planes, radius=16):
    """planes (n, h, w) float32 -> mv (n, nby, nbx, 2) int16 = (dx, dy), sad (n, nby, nbx, 5) int32, activity (n, nby, nbx) int32."""
    planes = np.asarray(planes, np.float32)
    n, h, w = planes.shape
    R = int(radius)
    nby, nbx = lattice(h, w, R)
    assert 1 <= R <= 16 and nby >= 1 and nbx >= 1
    q = quant(planes)
    mv = np.zeros((n, nby, nbx, 2), np.int16)
    sad = np.zeros((n, nby, nbx, 5), np.int32)
    act = np.zeros((n, nby, nbx), np.int32)
    cand, rank = candidates(R)
    side = 2 * R + 1
    Py = np.kron(np.eye(nby, dtype=np.float32), np.ones((1, B), np.float32))   # (nby, 16 nby): sums the rows of each block
    Px = np.kron(np.eye(nbx, dtype=np.float32), np.ones((B, 1), np.float32))
    for t in range(n):
        act[t] = activity_of(q[t], R)
        if t == 0:
            continue
        cur = np.ascontiguousarray(q[t, R:R + B * nby, R:R + B * nbx])
        prev = q[t - 1]
        S = np.empty((len(cand), nby, nbx), np.int64)
        for i, (dy, dx) in enumerate(cand):
            p = prev[R + dy:R + dy + B * nby, R + dx:R + dx + B * nbx]
            d = (np.maximum(cur, p) - np.minimum(cur, p)).astype(np.float32)   # |cur - p| without leaving uint8
            S[i] = (Py @ d @ Px).astype(np.int64)   # the blocks' sums; exact in float32: integers below 2^24 throughout
        assert S.max() <= 65280 and rank.max() <= 1088
        key = S * 2048 + rank[:, None, None]
        best = key.argmin(0)
        Sg = S.reshape(side, side, nby, nbx)
        for by in range(nby):
            for bx in range(nbx):
                cy, cx = divmod(int(best[by, bx]), side)
                mv[t, by, bx] = (cx - R, cy - R)
                for k, (oy, ox) in enumerate(((0, 0), (0, -1), (0, 1), (-1, 0), (1, 0))):
                    y, x = cy + oy, cx + ox
                    sad[t, by, bx, k] = Sg[y, x, by, bx] if 0 <= y < side and 0 <= x < side else -1
    return mv, sad, act


def _sum(values, order):
    """The float64 sum of a sequence in one of three orders."""
    v = [float(x) for x in values]
    if order == "reverse":
        v = v[::-1]
    if order == "pairwise":
        while len(v) > 1:
            v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
        return v[0] if v else 0.0
    s = 0.0
    for x in v:
        s += x
    return s


def subpixel(sad_row):
    """(offx, offy) from S at the best candidate and its neighbours: 0.5 (l - h) / (l - 2c + h), clipped to +-0.5; 0 without both neighbours,
    with a denominator that is not positive, or at an exact match (c = 0), whose vector is the whole-pixel one."""
    c = int(sad_row[0])
    out = []
    for ax in range(2):
        lo, hi = int(sad_row[1 + 2 * ax]), int(sad_row[2 + 2 * ax])
        den = lo - 2 * c + hi
        f = 0.5 * float(lo - hi) / float(den) if c > 0 and lo >= 0 and hi >= 0 and den > 0 else 0.0
        out.append(min(0.5, max(-0.5, f)))
    return out


def fit_pair(mv, sad, act, h, w, radius, min_activity=2000, order="forward", margins=None):
    """One pair's (a, b, tx, ty) and inlier count from its blocks' (nby, nbx, ...) arrays.  margins (a list): gets, per round 1 and 2 and per
    valid block, the relative distance of its squared residual from the round's threshold."""
    R = int(radius)
    nby, nbx = mv.shape[:2]
    cx0, cy0 = 0.5 * (w - 1), 0.5 * (h - 1)
    blocks = []
    for i in range(nby * nbx):
        by, bx = divmod(i, nbx)
        dxi, dyi = int(mv[by, bx, 0]), int(mv[by, bx, 1])
        if act[by, bx] < min_activity or abs(dxi) >= R or abs(dyi) >= R:
            continue
        s = [int(v) for v in sad[by, bx]]
        if 2 * ((s[1] - 2 * s[0] + s[2]) + (s[3] - 2 * s[0] + s[4])) < int(act[by, bx]):   # not sharp: a chance match, S flat around it
            continue
        ox, oy = subpixel(sad[by, bx])
        blocks.append(((R + B * bx + 7.5) - cx0, (R + B * by + 7.5) - cy0, dxi + ox, dyi + oy))
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
        if n < MIN_BLOCKS:
            return nan, 0
        s0 = float(n)
        sx, sy = _sum((b[0] for b in used), order), _sum((b[1] for b in used), order)
        sq = _sum((b[0] * b[0] + b[1] * b[1] for b in used), order)
        sdx, sdy = _sum((b[2] for b in used), order), _sum((b[3] for b in used), order)
        c = _sum((b[0] * b[2] + b[1] * b[3] for b in used), order)
        d = _sum((b[0] * b[3] - b[1] * b[2] for b in used), order)
        den = sq - (sx * sx + sy * sy) / s0
        if not den > 0.0:
            return nan, 0
        a1 = (c - (sx * sdx + sy * sdy) / s0) / den
        bb = (d - (sx * sdy - sy * sdx) / s0) / den
        tx = ((sdx - a1 * sx) + bb * sy) / s0
        ty = ((sdy - bb * sx) - a1 * sy) / s0
        fit = (a1, bb, tx, ty)
        if rnd < 2:
            thr = max(1.0, 4.0 * (_sum((res2(fit, b) for b in used), order) / s0))
    return (1.0 + fit[0], fit[1], fit[2], fit[3]), n


def motion_fit(mv, sad, act, h, w, radius=16, min_activity=2000, order="forward", margins=None):
    """motion (n, 4) float64 = (a, b, tx, ty) and inliers (n,) int32; row 0 is (1, 0, 0, 0) with 0 inliers."""
    n = mv.shape[0]
    motion = np.zeros((n, 4), np.float64)
    inl = np.zeros((n,), np.int32)
    for t in range(n):
        if t == 0:
            motion[0] = (1.0, 0.0, 0.0, 0.0)
            continue
        motion[t], inl[t] = fit_pair(mv[t], sad[t], act[t], h, w, radius, min_activity, order, margins)
    return motion, inl


def global_motion(planes, radius=16, min_activity=2000, order="forward"):
    planes = np.asarray(planes, np.float32)
    mv, sad, act = block_motion(planes, radius)
    return motion_fit(mv, sad, act, planes.shape[1], planes.shape[2], radius, min_activity, order)


def signal_score(v):
    """One signal's score over a scene: v[k], k = 1 .. m-1, the motion of pair k (v[0] is not read).  The path p[0] = 0, p[k] = p[k-1] + v[k],
    minus the straight line through its end points; E = |FFT(p)|^2 over bins 1 .. m//2 - 1; the first five bins over all of them, 1.0 when
    the total is 0."""
    v = np.asarray(v, np.float64)
    m = len(v)
    p = np.zeros(m, np.float64)
    for k in range(1, m):
        p[k] = p[k - 1] + v[k]
    p = p - (p[0] + (p[m - 1] - p[0]) * (np.arange(m, dtype=np.float64) / float(m - 1)))
    e = np.abs(np.fft.fft(p)) ** 2
    e = e[1:m // 2]
    total = float(e.sum())
    return 1.0 if total == 0.0 else float(e[:5].sum()) / total


def stability_scores(motion, scene_cuts=None, min_frames=24):
    """Per scene [a, b): translation = min(score of tx, score of ty), rotation = score of atan2(b, a), stability = the smaller; NaN for a scene
    of fewer than 24 frames or with a NaN pair (the pair at a cut does not count).  The clip: the frame-weighted mean of the scored scenes."""
    motion = np.asarray(motion, np.float64)
    T = motion.shape[0]
    edges = [0] + [int(c) for c in (scene_cuts or [])] + [T]
    scenes = []
    for a, b in zip(edges[:-1], edges[1:]):
        m = b - a
        rows = motion[a:b]
        if m < min_frames or not np.isfinite(rows[1:]).all():
            tr = ro = math.nan
        else:
            tr = min(signal_score(rows[:, 2]), signal_score(rows[:, 3]))
            ro = signal_score(np.arctan2(rows[:, 1], rows[:, 0]))
        scenes.append({"start": a, "end": b, "translation": tr, "rotation": ro, "stability": min(tr, ro) if tr == tr else math.nan})

    def clip(key):
        ok = [s for s in scenes if s[key] == s[key]]
        return sum(s[key] * (s["end"] - s["start"]) for s in ok) / sum(s["end"] - s["start"] for s in ok) if ok else math.nan
    return {"stability": clip("stability"), "translation": clip("translation"), "rotation": clip("rotation"), "scenes": scenes}


# ---------------------------------------------------------------------------------------------------------------- synthetic clips

def rolled_noise(shifts, h, w, seed):
    """Planes of seeded uint8 noise: plane t is plane t-1 rolled so that the block search finds (dx, dy) = shifts[t] (shifts[0] is not
    read); float32 in [-1, 1] at values that quantise back to the noise."""
    rs = np.random.RandomState(seed)
    base = rs.randint(0, 256, (h, w)).astype(np.uint8)
    out = [base]
    for dx, dy in shifts[1:]:
        out.append(np.roll(out[-1], (-dy, -dx), (0, 1)))   # cur[y, x] = prev[y + dy, x + dx]
    u8 = np.stack(out)
    return (u8.astype(np.float32) / np.float32(127.5) - np.float32(1)).astype(np.float32)


def planted_path(n, seed, jitter=True, pan=(0.8, 0.3), rot_deg=0.05, sigma_px=2.0, sigma_deg=0.3):
    """Per-frame poses (theta [rad], tx, ty): a steady pan and rotation, plus Gaussian pose jitter."""
    rs = np.random.RandomState(seed)
    k = np.arange(n, dtype=np.float64)
    th, tx, ty = np.deg2rad(rot_deg) * k, pan[0] * k, pan[1] * k
    if jitter:
        tx = tx + rs.normal(0.0, sigma_px, n)
        ty = ty + rs.normal(0.0, sigma_px, n)
        th = th + np.deg2rad(rs.normal(0.0, sigma_deg, n))
    return np.stack([th, tx, ty], 1)


def texture_clip(poses, h, w, seed):
    """Planes of an analytic texture -- 24 sinusoids with wavelengths from 5 to 48 pixels -- seen under the poses: pixel p (relative to the
    plane centre) of frame t shows the texture at Rot(theta_t) p + T_t, evaluated there, so nothing is resampled.  float32 in about [-1, 1]."""
    rs = np.random.RandomState(seed)
    lam = rs.uniform(5.0, 48.0, 24)
    ang = rs.uniform(0.0, 2 * np.pi, 24)
    ph = rs.uniform(0.0, 2 * np.pi, 24)
    kx, ky = 2 * np.pi / lam * np.cos(ang), 2 * np.pi / lam * np.sin(ang)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64) - 0.5 * (h - 1), np.arange(w, dtype=np.float64) - 0.5 * (w - 1), indexing="ij")
    out = np.empty((len(poses), h, w), np.float32)
    for t, (th, tx, ty) in enumerate(poses):
        X = math.cos(th) * xx - math.sin(th) * yy + tx
        Y = math.sin(th) * xx + math.cos(th) * yy + ty
        v = np.zeros((h, w), np.float64)
        for i in range(24):
            v += np.sin(kx[i] * X + ky[i] * Y + ph[i])
        out[t] = (0.11 * v).astype(np.float32)
    return out


def expected_motion(poses):
    """(n, 3) = (rotation [rad], tx, ty) that the fit should find for pair t: the point of frame t-1 that shows what p shows in frame t is
    Rot(theta_t - theta_{t-1}) p + Rot(-theta_{t-1}) (T_t - T_{t-1}).  Row 0 is zero."""
    out = np.zeros((len(poses), 3), np.float64)
    for t in range(1, len(poses)):
        th0, th1 = poses[t - 1][0], poses[t][0]
        dx, dy = poses[t][1] - poses[t - 1][1], poses[t][2] - poses[t - 1][2]
        out[t] = (th1 - th0, math.cos(th0) * dx + math.sin(th0) * dy, -math.sin(th0) * dx + math.cos(th0) * dy)
    return out
