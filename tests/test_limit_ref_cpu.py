"""CPU tests of the float64 restatement of crop-bounded smoothing (tests/limit_ref.py), against closed forms and brute force: the GPU tests
hold the kernels to this restatement, these hold the restatement to the definition."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limit_ref as L  # noqa: E402
import path_ref as P  # noqa: E402

FRAME = (360, 640)


def similarity(deg, scale, tx, ty):
    c, s = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    return [c, -s, tx, s, c, ty]


def test_the_ends_of_the_scale_are_the_identity_and_the_row():
    d = np.array([similarity(3.0, 1.04, 7.5, -2.25), similarity(-1.0, 0.97, -0.0, 11.0), [float("nan"), 0, 0, 0, 1, 0]])
    for levels in (1, 16, 64):
        table = L.levels_table(d, levels)
        assert table.shape == (3, levels + 1, 6)
        for t in (0, 1):
            assert tuple(table[t, 0]) == P.IDENTITY and not np.signbit(table[t, 0]).any()
            assert table[t, levels].tobytes() == d[t].tobytes()
            assert np.allclose(L.level_row(d[t], 1.0), d[t], rtol=1e-14, atol=1e-14)   # the formulas reach the row at lam = 1
        # a row that is not finite is its own every level, level 0 included
        assert all(table[2, l].tobytes() == d[2].tobytes() for l in range(levels + 1))
    # D(lam) D(1 - lam) = D: the levels lie on one geodesic of the linear part
    a, b = np.array(L.level_row(d[0], 0.25)), np.array(L.level_row(d[0], 0.75))
    A, B = a.reshape(2, 3)[:, :2], b.reshape(2, 3)[:, :2]
    assert np.allclose(A @ B, d[0].reshape(2, 3)[:, :2], rtol=1e-13, atol=1e-13)


def test_a_pure_translation_scales_linearly():
    d = [1.0, 0.0, 12.5, 0.0, 1.0, -40.0]
    for lam in (0.125, 0.5, 0.9):
        assert L.level_row(d, lam) == (1.0, 0.0, lam * 12.5, 0.0, 1.0, lam * -40.0)


def test_need_follows_the_prefix_rule():
    d = np.array([P.IDENTITY] * 6, np.float64)
    d[5, 2] = float("inf")
    counts = np.array([[0, 0, 0, 0, 0], [0, 0, 3, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 9], [0, 7, 0, 0, 0], [5, 5, 5, 5, 5]])
    assert L.need_of(counts, d).tolist() == [4, 1, -1, 3, 0, 4]   # (a level that is feasible behind an infeasible one does not count)
    d_out, strength, need = L.limit(d, counts, 4, 1.0)
    assert strength.tolist() == [1.0, 0.25, 0.0, 0.75, 0.0, 1.0]


def brute(s, relax, cuts):
    edges = [0] + list(cuts) + [len(s)]
    out = np.empty(len(s))
    for a, b in zip(edges[:-1], edges[1:]):
        for t in range(a, b):
            out[t] = min(s[u] + relax * abs(t - u) for u in range(a, b))
    return out


def test_the_sweeps_are_the_brute_force_envelope_and_never_cross_a_cut():
    rs = np.random.RandomState(3)
    for n, relax, cuts in ((1, 0.25, []), (40, 1.0 / 12, []), (40, 1.0 / 12, [7, 8, 30]), (300, 1.0 / 64, [150]), (25, 1.0, [])):
        s = rs.randint(0, 17, n) / 16.0
        got = L.sweeps(s, relax, cuts)
        assert np.allclose(got, brute(s, relax, cuts), rtol=0, atol=1e-12)
        assert (got <= s).all() and (got >= 0).all()
        edges = [0] + list(cuts) + [n]
        for a, b in zip(edges[:-1], edges[1:]):
            assert (np.abs(np.diff(got[a:b])) <= relax + 1e-12).all()
    # a frame at 0 on one side of a cut leaves the other side alone
    s = np.array([1.0, 1.0, 1.0, 0.0, 1.0, 1.0])
    assert L.sweeps(s, 0.25, [3]).tolist() == [1.0, 1.0, 1.0, 0.0, 0.25, 0.5]
    assert L.sweeps(s, 0.25).tolist() == [0.75, 0.5, 0.25, 0.0, 0.25, 0.5]


def test_the_rectangle_holds_every_cell_the_window_touches():
    assert L.rectangle(1.0, FRAME, (256, 256)) == (0, 255, 0, 255)
    for k in (0.97, 0.9, 0.5):
        for lat in ((256, 256), (19, 37), (2, 2)):
            i0, i1, j0, j1 = L.rectangle(k, FRAME, lat)
            # the window's outermost output pixel centres, on the lattice's scale, lie inside [j0, j1] x [i0, i1] ...
            for size, n, a, b in ((FRAME[1], lat[1], j0, j1), (FRAME[0], lat[0], i0, i1)):
                first = (0.5 * size - 0.5 * k * size + 0.5 * k - 0.5) * (n - 1) / (size - 1)
                last = (0.5 * size + 0.5 * k * size - 0.5 * k - 0.5) * (n - 1) / (size - 1)
                assert a <= first + 1e-4 and last - 1e-4 <= b and 0 <= a <= b <= n - 1
                assert a >= math.floor(first) - 1 and b <= math.ceil(last) + 1   # ... and no more than their cells


def test_need_on_an_identity_field_is_the_closed_form():
    """The identity field under align_corners=True maps node j to frame pixel x_j, and a translation composes exactly: node j samples
    x_j + lam tx.  The outermost nodes of the rectangle decide: the largest level with x_j0 + lam tx >= 0, x_j1 + lam tx <= W0 - 1, and y
    alike."""
    lat, levels, k = (19, 37), 16, 0.8   # (a rectangle inside the lattice: a rim node of the identity field lies ON the threshold)
    fh, fw = lat
    u, v = np.meshgrid(np.linspace(-1, 1, fw), np.linspace(-1, 1, fh))
    shifts = [(30.3, 0.0), (-61.7, 0.0), (0.0, 25.1), (0.0, -47.9), (44.4, -31.3), (3.0, 2.0), (1e4, 0.0)]
    field = np.stack([np.stack([u, v], -1)] * len(shifts)).astype(np.float64)
    d = np.array([[1.0, 0.0, tx, 0.0, 1.0, ty] for tx, ty in shifts])
    rect = L.rectangle(k, FRAME, lat)
    lo, hi, share = L.reach_bounds(field, L.levels_table(d, levels), FRAME, rect, True, 0)
    assert share == 0.0   # (the shifts keep every level away from a threshold)
    need = L.need_of(lo, d)
    i0, i1, j0, j1 = rect
    xs, ys = np.arange(fw) * (FRAME[1] - 1) / (fw - 1), np.arange(fh) * (FRAME[0] - 1) / (fh - 1)
    for t, (tx, ty) in enumerate(shifts):
        room = []
        if tx:
            room.append((xs[j0] if tx < 0 else FRAME[1] - 1 - xs[j1]) / abs(tx))
        if ty:
            room.append((ys[i0] if ty < 0 else FRAME[0] - 1 - ys[i1]) / abs(ty))
        want = min(levels, int(math.floor(levels * min(room))))
        assert need[t] == want, (t, need[t], want)
    assert need[5] == levels and need[6] == 0 and any(0 < v < levels for v in need)
