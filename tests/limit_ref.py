"""numpy float64 restatement of crop-bounded smoothing (csrc/path_limit.hip, csrc/field_reach.hip; stream.limit_path): the correction scaled
back to a share of itself, the table of levels, the count of a rectangle's uncovered nodes per level -- as bounds, through
path_ref.compose64 / shutter_ref.compose_rows64 and path_ref.uncovered_bounds -- the prefix rule, the two sweeps and the limited corrections."""
import math

import numpy as np

import path_ref as P
import shutter_ref as S


def level_row(d, lam):
    """D(lam) of one row d (6,): exp(lam ls) Rot(lam phi), lam (d2, d5); exactly the identity at 0; a row that is not finite is itself."""
    d = [float(v) for v in d]
    if not all(math.isfinite(v) for v in d):
        return tuple(d)
    if lam == 0.0:
        return P.IDENTITY
    ls, phi = math.log(math.hypot(d[0], d[3])), math.atan2(d[3], d[0])
    s, c, sn = math.exp(lam * ls), math.cos(lam * phi), math.sin(lam * phi)
    return (s * c, 0.0 - s * sn, lam * d[2], s * sn, s * c, lam * d[5])


def levels_table(d, levels):
    """table (n, levels+1, 6): level l = D(l / levels); the last level is the row verbatim."""
    d = np.asarray(d, np.float64)
    table = np.empty((d.shape[0], levels + 1, 6), np.float64)
    for t in range(d.shape[0]):
        for l in range(levels):
            table[t, l] = level_row(d[t], l / levels)
        table[t, levels] = d[t]
    return table


def rectangle(fraction, frame_hw, field_hw):
    """stream.limit_rectangle restated: (i0, i1, j0, j1) from the float32 zoom coefficients of the centred window."""
    h, w = frame_hw
    fh, fw = field_hw
    k = float(fraction)
    x0, x1, y0, y1 = 0.5 * w - 0.5 * k * w, 0.5 * w + 0.5 * k * w, 0.5 * h - 0.5 * k * h, 0.5 * h + 0.5 * k * h
    bx, by = (x1 - x0) / w, (y1 - y0) / h
    ax, ay = (x0 + 0.5 * bx - 0.5) * (fw - 1) / (w - 1), (y0 + 0.5 * by - 0.5) * (fh - 1) / (h - 1)
    ax, bx, ay, by = (float(np.float32(v)) for v in (ax, bx, ay, by))

    def span(a, b, n):
        hi = float(np.float32(b * (n - 1) + a))   # (the float64 sum of these float32 operands is exact: one rounding, fmaf's)
        return min(max(int(math.floor(a)), 0), n - 1), min(max(int(math.ceil(hi)), 0), n - 1)
    return span(ay, by, fh) + span(ax, bx, fw)


def reach_bounds(field, table, frame_hw, rect, align_corners, m, rates=None, r=0.0):
    """(lo, hi) (n, L+1) int64: the kernel's counts[t, l] lies in [lo, hi] -- path_ref.uncovered_bounds on the rectangle of the float64
    composition with table[:, l] -- and the share of (frame, level) pairs that the reference leaves undecided (lo < hi)."""
    table = np.asarray(table, np.float64)
    n, nl = table.shape[:2]
    i0, i1, j0, j1 = rect
    lo, hi = np.zeros((n, nl), np.int64), np.zeros((n, nl), np.int64)
    for l in range(nl):
        if rates is not None and float(r) != 0.0:
            out, tol = S.compose_rows64(field, table[:, l], np.asarray(rates, np.float64), r, frame_hw, return_terms=True)
        else:
            out, tol = P.compose64(field, table[:, l], frame_hw, return_terms=True)
        lo[:, l], hi[:, l], _ = P.uncovered_bounds(out[:, i0:i1 + 1, j0:j1 + 1], tol[:, i0:i1 + 1, j0:j1 + 1], frame_hw, align_corners, m)
    return lo, hi, float((lo < hi).mean())


def need_bounds(field, d, levels, frame_hw, rect, align_corners, m, frames, rates=None, r=0.0):
    """(need_lo, need_hi) for the listed frames (finite rows of d): the levels are walked upward and a frame stops at the first level at
    which even the reference's lower bound is not zero -- by the prefix rule nothing behind it matters.  need_lo counts every undecided
    node as uncovered (the smallest level the kernel may report), need_hi none."""
    d = np.asarray(d, np.float64)
    need_lo, need_hi = [], []
    for t in frames:
        table = levels_table(d[t:t + 1], levels)
        first_hi = first_lo = levels + 1   # the first level with hi > 0 / lo > 0
        for l in range(levels + 1):
            lo, hi, _ = reach_bounds(field[t:t + 1], table[:, l:l + 1], frame_hw, rect, align_corners, m,
                                     None if rates is None else np.asarray(rates)[t:t + 1], r)
            if hi[0, 0] > 0:
                first_hi = min(first_hi, l)
            if lo[0, 0] > 0:
                first_lo = l
                break
        need_lo.append(first_hi - 1)
        need_hi.append(first_lo - 1)
    return np.array(need_lo, np.int32), np.array(need_hi, np.int32)


def need_of(counts, d):
    """need (n,): the largest l with counts[t, l'] == 0 for every l' <= l, -1 if counts[t, 0] > 0; levels for a row of d that is not finite."""
    counts, d = np.asarray(counts), np.asarray(d, np.float64)
    n, nl = counts.shape
    need = np.empty(n, np.int32)
    for t in range(n):
        if not np.isfinite(d[t]).all():
            need[t] = nl - 1
            continue
        l = -1
        while l < nl - 1 and counts[t, l + 1] == 0:
            l += 1
        need[t] = l
    return need


def sweeps(s, relax, cuts=None):
    """The largest sequence below s that changes by at most relax per frame inside each scene: stream.zoom_schedule's two sweeps."""
    k = [float(v) for v in s]
    edges = [0] + [int(c) for c in (cuts or [])] + [len(k)]
    for a, b in zip(edges[:-1], edges[1:]):
        for t in range(a + 1, b):
            k[t] = min(k[t], k[t - 1] + relax)
        for t in range(b - 2, a - 1, -1):
            k[t] = min(k[t], k[t + 1] + relax)
    return np.array(k, np.float64)


def limit(d, counts, levels, relax, cuts=None):
    """(d_out (n, 6), strength (n,), need (n,)) from the counts: pws_path_limit, scene by scene."""
    d = np.asarray(d, np.float64)
    need = need_of(counts, d)
    strength = sweeps(np.maximum(need, 0) / float(levels), relax, cuts)
    d_out = np.array([d[t] if strength[t] == 1.0 else level_row(d[t], strength[t]) for t in range(d.shape[0])], np.float64).reshape(-1, 6)
    return d_out, strength, need


def limit_path(d, field, frame_hw, fraction, levels=16, relax=1.0, cuts=None, rates=None, r=0.0, align_corners=False, m=0, pessimistic=True):
    """stream.limit_path on the reference's counts: the upper bounds (pessimistic: the smallest need the kernel may report) or the lower
    ones.  Returns (d_out, strength, need, (lo, hi) of the rectangle's uncovered nodes under d_out)."""
    rect = rectangle(fraction, frame_hw, np.asarray(field).shape[1:3])
    lo, hi, _ = reach_bounds(field, levels_table(d, levels), frame_hw, rect, align_corners, m, rates, r)
    d_out, strength, need = limit(d, hi if pessimistic else lo, levels, relax, cuts)
    left = reach_bounds(field, d_out[:, None, :], frame_hw, rect, align_corners, m, rates, r)
    return d_out, strength, need, (left[0][:, 0], left[1][:, 0])
