"""numpy float64 restatement of the L1-optimal camera path (csrc/path_l1.hip; include/pwstable.h pws_l1_path has the definition): the scan
of the measured pose (tests/path_ref.py's), per component the primal-dual interior-point method on the LP

    minimise  w1 |D1 (x + q)|_1 + w2 |D2 (x + q)|_1 + w3 |D3 (x + q)|_1   subject to  -1 <= x <= 1,      x = (p^ - P) / b,  q = P / b,

and the corrections D[k] = C_k^-1 o C^_k.  Every product and sum is written in the kernel's order -- the reductions too: 256 partial sums
over the frames i = tid, tid + 256, ..., then a halving tree -- so that the two differ only where the device's exp / log / sin / cos / atan2
differ from the host's in the scan and in D.  NumPy only."""
import math

import numpy as np

import path_ref

THREADS = 256
MU = 10.0
MAX_STEPS = 64
TOL = 1e-9
PIVOT_FLOOR = 2.0 ** -44   # a pivot below this share of its diagonal entry is rounding noise: the row is skipped
PIVOT_HUGE = 1e128
COEF = {1: (-1.0, 1.0), 2: (1.0, -2.0, 1.0), 3: (-1.0, 3.0, -3.0, 1.0)}   # the k-th forward difference, row j over columns j .. j + k
WEIGHTS = (10.0, 1.0, 100.0)


def bounds(reach, frame_hw):
    """The box's half-widths b = (-log(1 - c), c min(H, W) / max(H, W), c W / 2, c H / 2), as stream.optimal_path forms them."""
    c, h, w = float(reach), int(frame_hw[0]), int(frame_hw[1])
    return (-math.log(1.0 - c), c * min(h, w) / max(h, w), c * w / 2.0, c * h / 2.0)


def diff(y, k):
    """The k-th forward difference of y, n - k rows, in the kernel's order of operations."""
    n = len(y)
    if k == 1:
        return y[1:] - y[:n - 1]
    if k == 2:
        return (y[:n - 2] - 2.0 * y[1:n - 1]) + y[2:]
    return ((y[3:] - 3.0 * y[2:n - 1]) + 3.0 * y[1:n - 2]) - y[:n - 3]


def ordered_sum(cols, n):
    """sum over i and over the columns, in the kernel's order: thread i % 256 adds its frames in ascending order and per frame the columns in
    the order given (a column shorter than n has no term there); then the partial sums are halved 128, 64, ..., 1."""
    acc = np.zeros(THREADS, np.float64)
    for base in range(0, n, THREADS):
        for c in cols:
            m = min(THREADS, len(c) - base)
            if m > 0:
                acc[:m] = acc[:m] + c[base:base + m]
    s = THREADS // 2
    while s >= 1:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return float(acc[0])


def dt_apply(cols, n):
    """sum_k (D_k^T cols[k])[i] for every i: k = 1, 2, 3 and per k the columns a = 0 .. k of row j = i - a, in that order."""
    out = np.zeros(n, np.float64)
    for k in (1, 2, 3):
        v = cols[k]
        for a in range(k + 1):
            out[a:a + n - k] = out[a:a + n - k] + COEF[k][a] * v   # rows j = 0 .. n-k-1 land on i = j + a
    return out


def band(theta, n):
    """The four diagonals A_d[i] = H[i, i + d] of sum_k D_k^T diag(theta_k) D_k: k = 1, 2, 3, per k the rows j = i - a for a = 0 .. k - d."""
    A = [np.zeros(n, np.float64) for _ in range(4)]
    for d in range(4):
        for k in (1, 2, 3):
            for a in range(0, k - d + 1):
                A[d][a:a + n - k] = A[d][a:a + n - k] + theta[k] * (COEF[k][a] * COEF[k][a + d])
    return A


def band_solve(A, rhs):
    """LDL^T without pivoting of the symmetric band (A[d][i] = H[i, i + d], d = 0 .. 3) and the two substitutions.  A pivot that is not above
    PIVOT_FLOOR times its diagonal entry is rounding noise (the band turns singular where the optimum is not unique): it is replaced by
    PIVOT_HUGE, which leaves that row's dx at 0 (S. Wright, SIAM J. Optim. 9, 1999).  Returns (dx, ok): ok is False when a pivot was not
    finite."""
    n = len(rhs)
    A0, A1, A2, A3 = A
    l1, l2, l3, w = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    D1 = D2 = D3 = 1.0      # D[i-1], D[i-2], D[i-3]
    l1p = l2p = l1pp = 0.0  # l1[i-1], l2[i-1], l1[i-2]
    z1 = z2 = z3 = 0.0
    ok = True
    with np.errstate(all="ignore"):
        for i in range(n):
            u3 = float(A3[i - 3]) if i >= 3 else 0.0
            a2 = float(A2[i - 2]) if i >= 2 else 0.0
            a1 = float(A1[i - 1]) if i >= 1 else 0.0
            c3 = np.float64(u3) / D3
            u2 = a2 - u3 * l1pp
            c2 = np.float64(u2) / D2
            u1 = (a1 - u3 * l2p) - u2 * l1p
            c1 = np.float64(u1) / D1
            D = ((float(A0[i]) - u3 * c3) - u2 * c2) - u1 * c1
            z = ((float(rhs[i]) - c1 * z1) - c2 * z2) - c3 * z3
            if not D > PIVOT_FLOOR * float(A0[i]):   # (also a NaN)
                ok = ok and bool(np.isfinite(D))
                D = PIVOT_HUGE
            l1[i], l2[i], l3[i], w[i] = c1, c2, c3, np.float64(z) / D
            D3, D2, D1 = D2, D1, D
            l1pp, l1p, l2p = l1p, float(c1), float(c2)
            z3, z2, z1 = z2, z1, z
        x1 = x2 = x3 = 0.0
        dx = np.zeros(n)
        for i in range(n - 1, -1, -1):
            c1 = l1[i + 1] if i + 1 < n else 0.0
            c2 = l2[i + 2] if i + 2 < n else 0.0
            c3 = l3[i + 3] if i + 3 < n else 0.0
            v = ((w[i] - c1 * x1) - c2 * x2) - c3 * x3
            dx[i] = v
            x3, x2, x1 = x2, x1, v
    return dx, ok


def solve_component(P, b, weights=WEIGHTS, trace=None):
    """One component of one scene: P (n,), half-width b > 0.  Returns (u (n,): p^ - P with |u| <= b exactly, info = (steps, eta, f,
    converged)); f is the scaled objective sum_k w_k sum e_k."""
    P = np.asarray(P, np.float64)
    n = len(P)
    if n <= 3:
        return np.zeros(n, np.float64), (0.0, 0.0, 0.0, 1.0)
    w = {1: float(weights[0]), 2: float(weights[1]), 3: float(weights[2])}
    wmax = max(w.values())
    q = P / b
    x = np.zeros(n)
    e, sp, sm, lp, lm = {}, {}, {}, {}, {}
    for k in (1, 2, 3):
        r = diff(q, k)
        e[k] = np.abs(r) + 1.0
        sp[k], sm[k] = e[k] - r, e[k] + r
        lp[k], lm[k] = 1.0 / sp[k], 1.0 / sm[k]
    sU, sL, lU, lL = np.ones(n), np.ones(n), np.ones(n), np.ones(n)
    m = float(8 * n - 12)
    steps, conv = 0, False
    with np.errstate(all="ignore"):
        while True:
            eta = ordered_sum([sp[1] * lp[1], sm[1] * lm[1], sp[2] * lp[2], sm[2] * lm[2], sp[3] * lp[3], sm[3] * lm[3], sU * lU, sL * lL], n)
            f = ordered_sum([w[1] * e[1], w[2] * e[2], w[3] * e[3]], n)
            rx = dt_apply({k: lp[k] - lm[k] for k in (1, 2, 3)}, n) + (lU - lL)
            re = {k: (w[k] - lp[k]) - lm[k] for k in (1, 2, 3)}
            res2 = ordered_sum([rx * rx, re[1] * re[1], re[2] * re[2], re[3] * re[3]], n)
            if trace is not None:
                trace.append((steps, eta, f, math.sqrt(res2)))
            if eta <= TOL * max(1.0, f) and math.sqrt(res2) <= TOL * max(1.0, wmax):
                conv = True
                break
            if steps == MAX_STEPS:
                break
            t = (MU * m) / max(eta, TOL * max(1.0, f))   # (held once the gap's criterion is met: the last steps only centre)
            gp, gm, vp, vm, G, be, th, y = {}, {}, {}, {}, {}, {}, {}, {}
            for k in (1, 2, 3):
                gp[k], gm[k] = lp[k] / sp[k], lm[k] / sm[k]
                vp[k], vm[k] = 1.0 / (t * sp[k]), 1.0 / (t * sm[k])
                G[k] = gp[k] + gm[k]
                th[k] = ((4.0 * gp[k]) * gm[k]) / G[k]
                be[k] = (vp[k] + vm[k]) - w[k]
                y[k] = (vp[k] - vm[k]) + ((gm[k] - gp[k]) * be[k]) / G[k]
            gU, gL, vU, vL = lU / sU, lL / sL, 1.0 / (t * sU), 1.0 / (t * sL)
            A = band(th, n)
            A[0] = A[0] + (gU + gL)
            rhs = (vL - vU) - dt_apply(y, n)
            dx, ok = band_solve(A, rhs)
            if not ok:
                break
            de, dsp, dsm, dlp, dlm = {}, {}, {}, {}, {}
            rmin, fin = math.inf, bool(np.isfinite(dx).all())
            pairs = []
            for k in (1, 2, 3):
                a = diff(dx, k)
                de[k] = (be[k] + (gp[k] - gm[k]) * a) / G[k]
                dsp[k], dsm[k] = de[k] - a, de[k] + a
                dlp[k], dlm[k] = (vp[k] - lp[k]) - gp[k] * dsp[k], (vm[k] - lm[k]) - gm[k] * dsm[k]
                pairs += [(sp[k], dsp[k]), (sm[k], dsm[k]), (lp[k], dlp[k]), (lm[k], dlm[k])]
                fin = fin and bool(np.isfinite(de[k]).all())
            dsU, dsL = 0.0 - dx, dx
            dlU, dlL = (vU - lU) + gU * dx, (vL - lL) - gL * dx
            pairs += [(sU, dsU), (sL, dsL), (lU, dlU), (lL, dlL)]
            for val, d in pairs:
                fin = fin and bool(np.isfinite(d).all())
                neg = d < 0.0
                if neg.any():
                    rmin = min(rmin, float((val[neg] / (0.0 - d[neg])).min()))
            alpha = min(1.0, 0.99 * rmin)
            if not (fin and math.isfinite(alpha)):
                break
            x = x + alpha * dx
            for k in (1, 2, 3):
                e[k] = e[k] + alpha * de[k]
                sp[k], sm[k] = sp[k] + alpha * dsp[k], sm[k] + alpha * dsm[k]
                lp[k], lm[k] = lp[k] + alpha * dlp[k], lm[k] + alpha * dlm[k]
            sU, sL, lU, lL = sU + alpha * dsU, sL + alpha * dsL, lU + alpha * dlU, lL + alpha * dlL
            steps += 1
    u = b * np.minimum(np.maximum(x, -1.0), 1.0)
    return u, (float(steps), eta, f, 1.0 if conv else 0.0)


def objective(p, weights=WEIGHTS):
    """w1 |D1 p|_1 + w2 |D2 p|_1 + w3 |D3 p|_1 in p's own units (a difference without rows is left out)."""
    p = np.asarray(p, np.float64)
    return float(sum(float(weights[k - 1]) * np.abs(diff(p, k)).sum() for k in (1, 2, 3) if len(p) > k))


def corrections(P, U):
    """D (n, 6), row-major 2 x 3: C_k^-1 o C^_k with P^ = P + U (path_ref.corrections, given the difference itself)."""
    D = np.zeros((P.shape[0], 6), np.float64)
    for k in range(P.shape[0]):
        lam, th = float(P[k, 0]), float(P[k, 1])
        dlam, dth, ux, uy = (float(v) for v in U[k])
        s, e, c, sn = math.exp(dlam), math.exp(-lam), math.cos(th), math.sin(th)
        D[k] = (s * math.cos(dth), 0.0 - s * math.sin(dth), e * (c * ux + sn * uy), s * math.sin(dth), s * math.cos(dth), e * (c * uy - sn * ux))
    return D


def l1_path(motion, bound, weights=WEIGHTS):
    """One scene: (path P (n, 4), U (n, 4) = P^ - P, D (n, 6), info (4, 4))."""
    P = path_ref.camera_path(motion)
    n = P.shape[0]
    U, info = np.zeros((n, 4), np.float64), np.zeros((4, 4), np.float64)
    for c in range(4):
        U[:, c], info[c] = solve_component(P[:, c], float(bound[c]), weights)
    if n <= 3:
        return P, U, np.tile(np.asarray(path_ref.IDENTITY, np.float64), (n, 1)), info
    return P, U, corrections(P, U), info


def optimal_path(motion, frame_hw, reach=0.1, weights=WEIGHTS, scene_cuts=None):
    """stream.optimal_path: (D (T, 6), path (T, 4), U (T, 4), info (scenes, 4, 4)), scene by scene."""
    motion = np.asarray(motion, np.float64)
    T = motion.shape[0]
    edges = [0] + [int(c) for c in (scene_cuts or [])] + [T]
    b = bounds(reach, frame_hw)
    D, P, U, infos = np.zeros((T, 6)), np.zeros((T, 4)), np.zeros((T, 4)), []
    for a, e in zip(edges[:-1], edges[1:]):
        P[a:e], U[a:e], D[a:e], info = l1_path(motion[a:e], b, weights)
        infos.append(info)
    return D, P, U, np.stack(infos) if infos else np.zeros((0, 4, 4))
