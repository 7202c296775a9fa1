"""GPU tests of the two small kernels of crop-bounded smoothing (csrc/path_limit.hip; C: pws_path_levels, pws_path_limit) against the
float64 restatement tests/limit_ref.py.

The table: levels 0 and `levels` are exact (the identity; the row's bytes), the levels between agree with float64 to 1e-14 relative -- the
device's log / hypot / atan2 / exp / cos / sin against the host's, a few ulp of 2.2e-16 each, on entries of size 1 to 100.  The sweeps and
d_out on hand-made counts are the reference's on the same counts: need and strength exactly (integers; sums and minima of the same
float64 operands in the same order), d_out to the same 1e-14 where it is computed and byte for byte where it is a copy."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limit_ref as L  # noqa: E402
import path_ref as P  # noqa: E402

EINVAL = -22
RTOL = 1e-14


def similarity(deg, scale, tx, ty):
    c, s = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    return [c, -s, tx, s, c, ty]


def rows(n, seed):
    """n similarities as pws_path_smooth writes them: a degree or two, a few per cent, tens of pixels."""
    rs = np.random.RandomState(seed)
    return np.array([similarity(rs.uniform(-2, 2), math.exp(rs.uniform(-0.05, 0.05)), rs.uniform(-60, 60), rs.uniform(-40, 40)) for _ in range(n)])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def p(t):
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else None


def levels_table(hip, d, levels):
    n = d.shape[0]
    table = torch.full((n, levels + 1, 6), 7.0, device="cuda", dtype=torch.float64)
    assert hip.lib().pws_path_levels(p(d), n, levels, p(table), hip.current_stream()) == 0, hip.lib().pws_last_error()
    return table


def path_limit(hip, d, counts, levels, relax):
    n = d.shape[0]
    need = torch.full((n,), -9, device="cuda", dtype=torch.int32)
    strength = torch.full((n,), -9.0, device="cuda", dtype=torch.float64)
    d_out = torch.full((n, 6), -9.0, device="cuda", dtype=torch.float64)
    rc = hip.lib().pws_path_limit(p(d), p(counts), n, levels, relax, p(need), p(strength), p(d_out), hip.current_stream())
    assert rc == 0, hip.lib().pws_last_error()
    return need, strength, d_out


def close(got, want):
    return np.abs(got - want) <= RTOL * np.maximum(np.abs(want), 1.0)


@pytest.mark.parametrize("levels", [1, 16, 64])
def test_the_table_against_float64(hip, levels):
    d = rows(70, levels)
    d[3] = P.IDENTITY
    d[5] = [1.0, 0.0, -12.5, 0.0, 1.0, 3.0]
    d[7, 2] = float("nan")
    d[9, 0] = float("inf")
    want = L.levels_table(d, levels)
    d_d = dev(d)
    got = levels_table(hip, d_d, levels).cpu().numpy()
    fin = np.isfinite(d).all(1)
    assert (got[fin, 0] == np.array(P.IDENTITY)).all() and not np.signbit(got[fin, 0]).any()   # level 0: exactly the identity
    assert got[:, levels].tobytes() == d.tobytes()                                              # the last level: the rows' bytes
    for t in np.flatnonzero(~fin):                                                               # rows that are not finite: every level
        assert all(got[t, l].tobytes() == d[t].tobytes() for l in range(levels + 1))
    err = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1.0)
    print("levels %d: largest relative error %.3g" % (levels, err.max()))
    assert close(got[fin], want[fin]).all()
    assert (got[5, :, [0, 1, 3, 4]] == np.array([[1.0], [0.0], [0.0], [1.0]])).all()           # a pure translation keeps its linear part
    again = levels_table(hip, d_d, levels).cpu().numpy()
    assert again.tobytes() == got.tobytes()


CASES = [(1, 16, 1.0 / 12), (300, 16, 1.0 / 12), (40, 1, 0.25), (40, 64, 1.0 / 64), (40, 16, 1.0), (257, 5, 0.07)]


@pytest.mark.parametrize("n,levels,relax", CASES, ids=["n%d-l%d-r%.3g" % c for c in CASES])
def test_the_sweeps_and_the_limited_rows_on_hand_made_counts(hip, n, levels, relax):
    rs = np.random.RandomState(n + levels)
    d = rows(n, n)
    counts = np.zeros((n, levels + 1), np.int32)
    for t in range(n):   # most frames feasible up to a random level, with junk behind it (the prefix rule must not read it as feasible)
        first = rs.randint(0, levels + 3)
        if first <= levels and rs.rand() < 0.4:
            counts[t, first] = rs.randint(1, 1000)
            counts[t, first + 1:] = rs.randint(0, 3, levels - first)
    if n > 8:
        counts[2, 0] = 5                      # need = -1
        counts[4] = 0                         # the whole correction
        d[6, 5] = float("nan")                # a row that is not finite: need = levels whatever the counts say
        counts[6] = 9
    want_d, want_s, want_need = L.limit(d, counts, levels, relax)
    d_d = dev(d)
    need, strength, d_out = path_limit(hip, d_d, dev(counts), levels, relax)
    need, strength, d_out = need.cpu().numpy(), strength.cpu().numpy(), d_out.cpu().numpy()
    assert (need == want_need).all()
    assert strength.tobytes() == want_s.tobytes()   # the same sums and minima of the same operands in the same order
    assert ((0 <= strength) & (strength <= 1)).all() and (np.abs(np.diff(strength)) <= relax + 1e-15).all()   # (the difference rounds once more)
    full = strength == 1.0
    assert d_out[full].tobytes() == d[full].tobytes()   # strength 1: the bytes of d
    if n > 8:
        assert need[2] == -1 and need[4] == levels and need[6] == levels and d_out[6].tobytes() == d[6].tobytes()
    fin = np.isfinite(d).all(1)
    assert close(d_out[fin], want_d[fin]).all()
    zero = fin & (strength == 0.0)
    assert (d_out[zero] == np.array(P.IDENTITY)).all()
    need2, strength2, d_out2 = path_limit(hip, d_d, dev(counts), levels, relax)
    assert torch.equal(need2.cpu(), torch.from_numpy(need)) and strength2.cpu().numpy().tobytes() == strength.tobytes()
    assert d_out2.cpu().numpy().tobytes() == d_out.tobytes()


def test_bad_arguments(hip):
    lib, s = hip.lib(), hip.current_stream()
    n, levels = 4, 8
    d = dev(rows(n, 1))
    table = torch.full((n, levels + 1, 6), 7.0, device="cuda", dtype=torch.float64)
    counts = torch.zeros((n, levels + 1), device="cuda", dtype=torch.int32)
    need = torch.full((n,), -9, device="cuda", dtype=torch.int32)
    strength = torch.full((n,), -9.0, device="cuda", dtype=torch.float64)
    d_out = torch.full((n, 6), -9.0, device="cuda", dtype=torch.float64)
    for lv in (0, -1, 65):
        assert lib.pws_path_levels(p(d), n, lv, p(table), s) == EINVAL and b"levels" in lib.pws_last_error()
        assert lib.pws_path_limit(p(d), p(counts), n, lv, 0.5, p(need), p(strength), p(d_out), s) == EINVAL
    assert lib.pws_path_levels(None, n, levels, p(table), s) == EINVAL and lib.pws_path_levels(p(d), n, levels, None, s) == EINVAL
    assert lib.pws_path_levels(p(d), -1, levels, p(table), s) == EINVAL
    assert lib.pws_path_levels(p(d.data_ptr() + 4), n, levels, p(table), s) == EINVAL and b"aligned" in lib.pws_last_error()
    for relax in (0.0, -0.5, 1.5, float("nan")):
        assert lib.pws_path_limit(p(d), p(counts), n, levels, relax, p(need), p(strength), p(d_out), s) == EINVAL and b"relax" in lib.pws_last_error()
    for k in range(5):
        args = [p(d), p(counts), p(need), p(strength), p(d_out)]
        args[k] = None
        assert lib.pws_path_limit(args[0], args[1], n, levels, 0.5, args[2], args[3], args[4], s) == EINVAL
    assert lib.pws_path_limit(p(d), p(counts), -1, levels, 0.5, p(need), p(strength), p(d_out), s) == EINVAL
    assert lib.pws_path_limit(p(d), p(counts), n, levels, 0.5, p(need), p(strength.data_ptr() + 4), p(d_out), s) == EINVAL
    # n = 0: nothing is launched, nothing is written (NULL pointers are fine)
    assert lib.pws_path_levels(p(d), 0, levels, p(table), s) == 0 and lib.pws_path_levels(None, 0, levels, None, s) == 0
    assert lib.pws_path_limit(p(d), p(counts), 0, levels, 0.5, p(need), p(strength), p(d_out), s) == 0
    assert lib.pws_path_limit(None, None, 0, levels, 0.5, None, None, None, s) == 0
    torch.cuda.synchronize()
    assert bool((table == 7.0).all()) and bool((need == -9).all()) and bool((strength == -9.0).all()) and bool((d_out == -9.0).all())
