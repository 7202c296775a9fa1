"""float64 restatement of the automatic crop (reference main_new.py:484-606) for the tests: the lattice, the fit of
csrc/homography.hip (Hartley-normalised DLT with m33 = 1, then Gauss-Newton on the forward reprojection error), the corners
and the window recurrence.  Written from the algorithm, not from the kernel: it solves with numpy and sums in numpy's order."""
import numpy as np

SIDE, STRIDE_Y, STRIDE_X = 20, 15, 30
CORNER = float(np.float32(0.992))          # the reference's corner points are an np.float32 array (main_new.py:572)
FLT_EPSILON = float(np.finfo(np.float32).eps)


def lattice(frame_hw):
    """(rows (400,), cols (400,), p2 (400, 2) float64 of the np.float32 values): point k = a * 20 + b."""
    h0, w0 = frame_hw
    a, b = np.divmod(np.arange(SIDE * SIDE), SIDE)
    r = h0 // 2 + (a - SIDE // 2) * STRIDE_Y
    c = w0 // 2 + (b - SIDE // 2) * STRIDE_X
    p2 = np.stack([(w0 / 2 + (b - SIDE / 2) * STRIDE_X) / w0 * 2 - 1, r / h0 * 2 - 1], 1).astype(np.float32)
    return r, c, p2.astype(np.float64)


def _normalise(p):
    c = p.mean(0)
    md = np.sqrt(((p - c) ** 2).sum(1)).mean()
    return c, md


def fit(p1, p2, iters=20, info=None):
    """M (3, 3), m33 = 1, minimising sum |p2 - pi(M [p1, 1])|^2; None where the kernel reports NaN.  ``info``: see fit_info."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    c1, md1 = _normalise(p1)
    c2, md2 = _normalise(p2)
    if info is not None:
        info.update(steps=0, pivot=np.inf, spread=md1 / (1e-6 * (1 + np.abs(c1).max())))
    if not (md1 > 1e-6 * (1 + np.abs(c1).max()) and md2 > 0):
        return None
    n1, n2 = np.sqrt(2) / md1, np.sqrt(2) / md2
    q1, q2 = (p1 - c1) * n1, (p2 - c2) * n2
    x, y, u, v = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    one, zero = np.ones_like(x), np.zeros_like(x)
    A = np.concatenate([np.stack([x, y, one, zero, zero, zero, -x * u, -y * u], 1),
                        np.stack([zero, zero, zero, x, y, one, -x * v, -y * v], 1)])
    h = _solve(A.T @ A, A.T @ np.concatenate([u, v]), info)
    if h is None:
        return None
    for _ in range(iters):
        iw = 1 / (h[6] * x + h[7] * y + 1)
        pu, pv = (h[0] * x + h[1] * y + h[2]) * iw, (h[3] * x + h[4] * y + h[5]) * iw
        xi, yi = x * iw, y * iw
        J = np.concatenate([np.stack([xi, yi, iw, zero, zero, zero, -xi * pu, -yi * pu], 1),
                            np.stack([zero, zero, zero, xi, yi, iw, -xi * pv, -yi * pv], 1)])
        d = _solve(J.T @ J, J.T @ np.concatenate([u - pu, v - pv]), info)
        if d is None:
            return None
        h = h + d
        if info is not None:
            info["steps"] += 1
        if np.abs(d).max() < 1e-12 * (1 + np.abs(h).max()):
            break
    Hn = np.append(h, 1.0).reshape(3, 3)
    T1 = np.array([[n1, 0, -n1 * c1[0]], [0, n1, -n1 * c1[1]], [0, 0, 1]])
    T2i = np.array([[1 / n2, 0, c2[0]], [0, 1 / n2, c2[1]], [0, 0, 1]])
    M = T2i @ Hn @ T1
    M = M / M[2, 2]
    return M if np.all(np.isfinite(M)) else None


def _solve(N, g, info=None):
    """Cholesky with the kernel's test: every pivot > 1e-12 x its diagonal entry."""
    n = N.shape[0]
    L = np.zeros_like(N)
    for i in range(n):
        for j in range(i + 1):
            s = N[j, i] - L[i, :j] @ L[j, :j]
            if i == j:
                if info is not None:
                    info["pivot"] = min(info["pivot"], s / N[i, i] if N[i, i] else 0.0)   # an empty column has no pivot at all
                if not s > 1e-12 * N[i, i]:
                    return None
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    return np.linalg.solve(L.T, np.linalg.solve(L, g))


def corners(M):
    """cv2.perspectiveTransform of the reference's four corner points (float32 output): (4, 2)."""
    pts = np.array([[-1, -1], [-1, CORNER], [CORNER, CORNER], [CORNER, -1]], np.float64)
    X = pts @ M[:2, :2].T + M[:2, 2]
    w = pts @ M[2, :2] + M[2, 2]
    iw = np.where(np.abs(w) > FLT_EPSILON, 1 / np.where(w == 0, 1, w), 0.0)
    return (X * iw[:, None]).astype(np.float32).astype(np.float64)


def bounds(M, frame_hw):
    """(top, bottom, left, right) in source pixels, NaN when the fit failed (main_new.py:575-603)."""
    if M is None:
        return np.full(4, np.nan)
    h0, w0 = frame_hw
    c = corners(M)
    X, Y = (c[:, 0] + 1) * w0 / 2, (c[:, 1] + 1) * h0 / 2
    b = np.array([max(Y[0], Y[3]), min(Y[1], Y[2]), max(X[0], X[1]), min(X[2], X[3])])
    return b if np.all(np.isfinite(b)) else np.full(4, np.nan)


def crop_window(bnds, frame_hw, period=30, rate=0.5):
    """The reference's recurrence (main_new.py:575-603) restated over the (T, 4) bounds: (x0, x1, y0, y1) in source pixels."""
    h0, w0 = frame_hw
    T, half = len(bnds), period // 2
    x0, x1, y0, y1 = 0.0, float(w0), 0.0, float(h0)
    for i in range(1, T):
        if half < i < T - half:
            top, bottom, left, right = (float(v) for v in bnds[i])
            y0 = y0 + (top - y0) * rate if y0 < top else y0
            y1 = y1 - (y1 - bottom) * rate if y1 > bottom else y1
            x0 = x0 + (left - x0) * rate if x0 < left else x0
            x1 = x1 - (x1 - right) * rate if x1 > right else x1
    return x0, x1, y0, y1


# ---- instruments of tests/test_homography_ref_cpu.py and tests/test_hip_homography_float64.py

def sample64(field, frame_hw):
    """The align_corners=True bilinear resize of ``field`` (fh, fw, 2) to the frame, at the 400 lattice points, in float64: (p1 (400, 2),
    the set of field nodes (y, x) that any sample's four taps read -- a tap of weight zero is still a tap)."""
    f = np.asarray(field, np.float64)
    fh, fw = f.shape[:2]
    h0, w0 = frame_hw
    r, c, _ = lattice(frame_hw)
    sy, sx = (fh - 1) / (h0 - 1) * r, (fw - 1) / (w0 - 1) * c
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    y1, x1 = y0 + (y0 < fh - 1), x0 + (x0 < fw - 1)
    ly, lx = (sy - y0)[:, None], (sx - x0)[:, None]
    p1 = (1 - ly) * ((1 - lx) * f[y0, x0] + lx * f[y0, x1]) + ly * ((1 - lx) * f[y1, x0] + lx * f[y1, x1])
    nodes = set()
    for ys, xs in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
        nodes.update(zip(ys.tolist(), xs.tolist()))
    return p1, nodes


def fit_info(p1, p2, iters=20):
    """``fit`` and what its margins were: (M or None, {"steps": Gauss-Newton steps taken, "pivot": the smallest s / N[i][i] seen in any
    Cholesky (inf before the first), "spread": md1 / (1e-6 (1 + max |c1|)), the no-spread test's ratio})."""
    info = {}
    return fit(p1, p2, iters, info), info


def fit_independent(p1, p2, iters=50):
    """The second reference: the same cost, sum |p2 - pi(M [p1, 1])|^2, minimised by Gauss-Newton in the raw coordinates with
    numpy.linalg.lstsq on the Jacobian itself, started from the plain DLT (the null vector of the 800 x 9 system by numpy.linalg.svd).
    It shares neither normalisation, normal equations, Cholesky nor start with ``fit``.  M (3, 3) with m33 = 1."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    x, y, u, v = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    one, zero = np.ones_like(x), np.zeros_like(x)
    A = np.concatenate([np.stack([x, y, one, zero, zero, zero, -x * u, -y * u, -u], 1),
                        np.stack([zero, zero, zero, x, y, one, -x * v, -y * v, -v], 1)])
    h = np.linalg.svd(A)[2][-1]
    h = h[:8] / h[8]
    for _ in range(iters):
        iw = 1 / (h[6] * x + h[7] * y + 1)
        pu, pv = (h[0] * x + h[1] * y + h[2]) * iw, (h[3] * x + h[4] * y + h[5]) * iw
        xi, yi = x * iw, y * iw
        J = np.concatenate([np.stack([xi, yi, iw, zero, zero, zero, -xi * pu, -yi * pu], 1),
                            np.stack([zero, zero, zero, xi, yi, iw, -xi * pv, -yi * pv], 1)])
        d = np.linalg.lstsq(J, np.concatenate([u - pu, v - pv]), rcond=None)[0]
        h = h + d
        if np.abs(d).max() <= 1e-15 * (1 + np.abs(h).max()):
            break
    return np.append(h, 1.0).reshape(3, 3)


def spread(p1, p2):
    """max |fit - fit_independent| over the entries of M: what two float64 solvers of the same problem leave open."""
    return float(np.abs(fit(p1, p2) - fit_independent(p1, p2)).max())


def gate(p1, p2):
    """How far a third float64 solver that sums in yet another order may be from either: 16 x the spread, at least 1e-12
    (tests/test_hip_motion.py's rule)."""
    return max(16.0 * spread(p1, p2), 1e-12)


FRAMES = [(300, 600), (301, 601), (361, 641), (1080, 1920), (2160, 3840)]   # the minimum, odd, odd, large, larger
FIELD_SIZES = [(256, 256), (2, 2), (5, 7), (64, 48), (33, 257)]
CASES = [(frame_hw, field_hw) for frame_hw in FRAMES for field_hw in FIELD_SIZES]   # one launch each, carrying every family
_PROJ = [[1.05, 0.02, -0.03], [0.01, 1.1, 0.02], [0.03, -0.02, 1.0]]
FAMILIES = {   # name: (P, eps, noise)
    "identity": ([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], 0.0, 0.0),
    "projective": (_PROJ, 0.01, 0.0),
    "strong": ([[0.9, 0.1, 0.05], [-0.08, 1.15, -0.04], [0.25, -0.2, 1.0]], 0.02, 0.0),
    "noisy": (_PROJ, 0.02, 0.03),
    "mirror": ([[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], 0.01, 0.0),
}


def _axes(field_hw):
    fh, fw = field_hw
    return np.meshgrid(np.linspace(-1, 1, fw), np.linspace(-1, 1, fh))   # xx, yy: (fh, fw); a single row or column sits at -1


def family_field(name, field_hw, phase=0.0, seed=0, horizon=1.0):
    """(fh, fw, 2) float32: node p samples the source at pi(P [p, 1]) + eps x a smooth residual (test_hip_auto_crop._field's) + noise x
    uniform(-1, 1), seeded by the size and ``seed``.  ``horizon`` scales P's projective row."""
    P, eps, noise = FAMILIES[name]
    xx, yy = _axes(field_hw)
    w = horizon * (P[2][0] * xx + P[2][1] * yy) + P[2][2]
    fx = (P[0][0] * xx + P[0][1] * yy + P[0][2]) / w + eps * np.sin(np.pi * xx + phase) * np.cos(0.5 * np.pi * yy)
    fy = (P[1][0] * xx + P[1][1] * yy + P[1][2]) / w + eps * np.cos(np.pi * yy - phase) * np.sin(0.7 * np.pi * xx)
    f = np.stack([fx, fy], -1)
    if noise:
        f = f + noise * np.random.RandomState(field_hw[0] * 1000 + field_hw[1] + seed).uniform(-1, 1, f.shape)
    return f.astype(np.float32)


# ``fit`` stops at a step below 1e-12 (1 + max |h|), as the kernel does.  Where Gauss-Newton converges linearly (a large residual: noise,
# or a strong homography held by four nodes), what remains after that step is up to 1.5e-12 in M, and fit_independent, which runs
# to 1e-15, sees it: measured on the 125 table entries as first built (phase k, seed 0, horizon 1), 115 spreads of 1.1e-16 .. 6.1e-14
# and the ten below.  A spread above 1e-12 / 16 would widen the kernel's gate past its 1e-12 floor, so those ten entries are REPLACED by
# their nearest neighbour that stays below half of it: the same frame, field size, matrix and eps, at the first phase k + j / 2 (strong) or
# seed j (noisy) that does, and, where no phase does (four nodes hold no residual to move), the projective row at half strength.
REPLACED = {   # (frame, field size, family): what changes   # spread as first built -> as replaced
    ((300, 600), (2, 2), "strong"): {"horizon": 0.5},         # 2.5e-13 -> 3.4e-14
    ((301, 601), (2, 2), "strong"): {"horizon": 0.5},         # 2.4e-13 -> 3.3e-14
    ((361, 641), (2, 2), "strong"): {"horizon": 0.5},         # 1.7e-13 -> 6.9e-15
    ((1080, 1920), (5, 7), "strong"): {"phase": 2.5},         # 1.2e-13 -> 2.3e-14
    ((1080, 1920), (64, 48), "noisy"): {"seed": 1},           # 1.4e-13 -> 6.7e-15
    ((2160, 3840), (256, 256), "noisy"): {"seed": 6},         # 1.0e-13 -> 2.0e-14
    ((2160, 3840), (5, 7), "strong"): {"phase": 4.5},         # 1.8e-13 -> 8.3e-15
    ((2160, 3840), (5, 7), "noisy"): {"seed": 9},             # 1.4e-13 -> 2.5e-14
    ((2160, 3840), (64, 48), "noisy"): {"seed": 38},          # 1.5e-12 -> 2.9e-14
    ((2160, 3840), (33, 257), "noisy"): {"seed": 5},          # 2.0e-13 -> 2.8e-14
}


def case_fields(frame_hw, field_hw):
    """(5, fh, fw, 2): the families in FAMILIES' order, family k at phase k, but for the entries of REPLACED."""
    return np.stack([family_field(name, field_hw, **{"phase": float(k), **REPLACED.get((frame_hw, field_hw, name), {})})
                     for k, name in enumerate(FAMILIES)])


def first_built(field_hw, name):
    """An entry of REPLACED as the table first had it: the GPU file still runs these, under the gate their own spread gives."""
    return family_field(name, field_hw, phase=float(list(FAMILIES).index(name)))


def _xy_field(fx, fy):
    return np.stack(np.broadcast_arrays(fx, fy), -1).astype(np.float32)


def nofit_fields(field_hw=(256, 256)):
    """Fields without a homography, by name.  "spread": every sample within 1e-8 of one point; "line", "x_only", "parabola": the
    samples lie on a curve, so the 8 x 8 normal matrix has no full rank."""
    xx, yy = _axes(field_hw)
    return {"constant": _xy_field(0.3 + 0 * xx, 0.3 + 0 * xx), "spread": _xy_field(1e-8 * xx, 1e-8 * yy), "line": _xy_field(xx, xx),
            "x_only": _xy_field(xx, 0.1 + 0 * xx), "parabola": _xy_field(xx, xx * xx)}


def near_fields(field_hw=(256, 256)):
    """Fields next to a no-fit one that still have a homography: a spread of 1e-5, and a line opened by 1e-3."""
    xx, yy = _axes(field_hw)
    return {"spread": _xy_field(1e-5 * xx, 1e-5 * yy), "line": _xy_field(xx, xx + 1e-3 * yy)}


def ulp32(v):
    """The spacing of float32 at |v|."""
    return float(np.spacing(np.abs(np.float32(v))))
