"""The float64 restatement of the L1-optimal path (tests/l1_path_ref.py) against linear programs solved by HiGHS (tests/golden/l1_path.npz,
written by tests/golden/make_golden_l1_path.py): the interior-point method that csrc/path_l1.hip runs is held to an independent solver's
optima before the kernel is held to the restatement."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import l1_path_ref as L  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "l1_path.npz"))
CASES = ("walk4", "walk5", "walk9", "walk200", "walk513", "ramp", "jolt", "constant", "shake", "angle")
_solved = {}


def solved(name):
    """(P, b, f_LP, u, info) of a case, solved once."""
    if name not in _solved:
        P, b = GOLDEN[name + "_P"], float(GOLDEN[name + "_b"])
        u, info = L.solve_component(P, b)
        _solved[name] = (P, b, float(GOLDEN[name + "_f"]), u, info)
    return _solved[name]


def test_the_fixture_holds_every_case():
    assert sorted(CASES) == sorted({k.rsplit("_", 1)[0] for k in GOLDEN.files})
    assert [len(GOLDEN[c + "_P"]) for c in CASES] == [4, 5, 9, 200, 513, 40, 60, 40, 60, 120]
    assert [float(GOLDEN[c + "_b"]) for c in CASES] == [20.0, 20.0, 20.0, 20.0, 15.0, 5.0, 20.0, 20.0, 5.0, 0.05]
    # HiGHS's own minimiser is feasible and has HiGHS's objective: the fixture is consistent in itself
    for c in CASES:
        P, b, f, p = GOLDEN[c + "_P"], float(GOLDEN[c + "_b"]), float(GOLDEN[c + "_f"]), GOLDEN[c + "_p"]
        assert np.abs(p - P).max() <= b + 1e-9 and abs(L.objective(p) - f) <= 1e-9 * max(1.0, f)


@pytest.mark.parametrize("name", CASES)
def test_feasible_optimal_and_converged(name):
    """|p^ - P| <= b exactly; the objective within 1e-6 f_LP + 1e-6 max(w) b of HiGHS's optimum (the stop rule bounds the gap by about 1e-9
    max(b, f): the gate leaves 1000 x); converged within 64 steps.  Measured: relative gaps 2.5e-12 .. 1.3e-10 where f_LP > 0 (ramp, walk200,
    walk513, jolt), 0 .. 8.5e-12 absolute where it is 0, in 15 .. 36 steps."""
    P, b, f_lp, u, info = solved(name)
    assert np.all(np.abs(u) <= b)
    f = L.objective(P + u)
    print("%s: n %d steps %d eta %.3g f %.12g f_LP %.12g gap %.3g" % (name, len(P), info[0], info[1], f, f_lp, f - f_lp))
    assert f - f_lp <= 1e-6 * f_lp + 1e-6 * max(L.WEIGHTS) * b
    assert info[3] == 1.0 and info[0] <= 64


def test_a_static_path_is_found_where_one_exists():
    """Shake inside the box, a constant, the short walks: the optimum is 0 and the path is static to rounding."""
    for name in ("shake", "constant", "walk4", "walk5", "walk9", "angle"):
        P, b, f_lp, u, _ = solved(name)
        assert f_lp == 0.0 and np.abs(np.diff(P + u)).max() <= 1e-9 * b


def test_the_path_is_made_of_parabolic_pieces():
    """n = 513: most third differences vanish.  Measured on this restatement: 34 of 510 above 1e-6 px (the largest 0.206 px), which is the
    gate."""
    P, b, _, u, _ = solved("walk513")
    d3 = np.abs(L.diff(P + u, 3))
    print("third differences above 1e-6 px: %d of %d, largest %.3g" % ((d3 > 1e-6).sum(), len(d3), d3.max()))
    assert (d3 > 1e-6).sum() <= 34


def test_short_scenes_keep_their_path():
    for n in range(4):
        motion = np.tile(np.array([1.0, 0.0, 3.0, -2.0]), (n, 1))
        P, U, D, info = L.l1_path(motion, (0.1, 0.1, 10.0, 10.0))
        assert not U.any() and all(tuple(row) == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0) for row in D)
        assert info.tolist() == [[0.0, 0.0, 0.0, 1.0]] * 4


def test_scenes_are_solved_on_their_own():
    rs = np.random.RandomState(3)
    motion = np.concatenate([np.ones((30, 1)), np.zeros((30, 1)), rs.normal(0.0, 2.0, (30, 2))], 1)
    D, P, U, info = L.optimal_path(motion, (200, 400), scene_cuts=[12])
    for a, b in ((0, 12), (12, 30)):
        D1, P1, U1, _ = L.optimal_path(motion[a:b], (200, 400))
        assert np.array_equal(D[a:b], D1) and np.array_equal(P[a:b], P1) and np.array_equal(U[a:b], U1)
    assert info.shape == (2, 4, 4) and (info[:, :, 3] == 1.0).all()
    assert L.bounds(0.1, (200, 400)) == (-math.log(1.0 - 0.1), 0.05, 20.0, 10.0)
