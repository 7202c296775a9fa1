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


def fit(p1, p2, iters=20):
    """M (3, 3), m33 = 1, minimising sum |p2 - pi(M [p1, 1])|^2; None where the kernel reports NaN."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    c1, md1 = _normalise(p1)
    c2, md2 = _normalise(p2)
    if not (md1 > 1e-6 * (1 + np.abs(c1).max()) and md2 > 0):
        return None
    n1, n2 = np.sqrt(2) / md1, np.sqrt(2) / md2
    q1, q2 = (p1 - c1) * n1, (p2 - c2) * n2
    x, y, u, v = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    one, zero = np.ones_like(x), np.zeros_like(x)
    A = np.concatenate([np.stack([x, y, one, zero, zero, zero, -x * u, -y * u], 1),
                        np.stack([zero, zero, zero, x, y, one, -x * v, -y * v], 1)])
    h = _solve(A.T @ A, A.T @ np.concatenate([u, v]))
    if h is None:
        return None
    for _ in range(iters):
        iw = 1 / (h[6] * x + h[7] * y + 1)
        pu, pv = (h[0] * x + h[1] * y + h[2]) * iw, (h[3] * x + h[4] * y + h[5]) * iw
        xi, yi = x * iw, y * iw
        J = np.concatenate([np.stack([xi, yi, iw, zero, zero, zero, -xi * pu, -yi * pu], 1),
                            np.stack([zero, zero, zero, xi, yi, iw, -xi * pv, -yi * pv], 1)])
        d = _solve(J.T @ J, J.T @ np.concatenate([u - pu, v - pv]))
        if d is None:
            return None
        h = h + d
        if np.abs(d).max() < 1e-12 * (1 + np.abs(h).max()):
            break
    Hn = np.append(h, 1.0).reshape(3, 3)
    T1 = np.array([[n1, 0, -n1 * c1[0]], [0, n1, -n1 * c1[1]], [0, 0, 1]])
    T2i = np.array([[1 / n2, 0, c2[0]], [0, 1 / n2, c2[1]], [0, 0, 1]])
    M = T2i @ Hn @ T1
    M = M / M[2, 2]
    return M if np.all(np.isfinite(M)) else None


def _solve(N, g):
    """Cholesky with the kernel's test: every pivot > 1e-12 x its diagonal entry."""
    n = N.shape[0]
    L = np.zeros_like(N)
    for i in range(n):
        for j in range(i + 1):
            s = N[j, i] - L[i, :j] @ L[j, :j]
            if i == j:
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
