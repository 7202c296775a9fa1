"""CPU tests of the rolling-shutter estimate's float64 restatement (tests/shutter_est_ref.py) on analytic rolling-shutter clips: row y of
frame t is exposed at t + r clamp(y / (h - 1), -1/2, 1/2) under shutter_ref's camera plus two faster shake components, the texture evaluated
at the exposed position, so nothing is resampled.  256 x 256, 32 frames, radius 16; block search and fit are motion_ref's.

What the estimate recovers, what it is worth end to end, what the gate refuses, and the bookkeeping of cuts and NaN rows.  Measured here
(printed by the tests): r_hat = 0.734 / 0.026 / -0.476 for r = 0.8 / 0.0 / -0.5 (seeds 7 / 8 / 9), -0.761 for r = -0.8; se 0.005 .. 0.010;
0.78 on the steady pan."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shutter_est_ref as E  # noqa: E402
import shutter_ref as S  # noqa: E402

BOUND = 0.1      # |r_hat - r|: a float64 prototype's worst case over nine runs was 0.066
MAX_SE = 0.02    # VideoStabilizer's default gate


@functools.lru_cache(maxsize=None)
def _clip(r, seed):
    """(estimate, terms, motion, blocks) of the analytic clip exposed under r; shared, read-only."""
    est, tm, motion, blocks = E.estimate_clip(E.rolling_clip(r, seed=seed), return_terms=True)
    for a in (est, tm, motion) + tuple(blocks):
        a.setflags(write=False)
    return est, tm, motion, blocks


def test_recovery_on_the_analytic_camera():
    for r, seed in ((0.8, 7), (0.0, 8), (-0.5, 9)):
        est = _clip(r, seed)[0]
        print("r", r, "seed", seed, "r_hat %.4f error %.4f se %.4f D %.1f blocks %d" % (est[0], est[0] - r, est[1], est[2], est[3]))
        assert abs(est[0] - r) <= BOUND, (r, est)
        assert est[1] <= MAX_SE and E.choose(est, MAX_SE) == min(1.0, max(-1.0, est[0]))   # these clips pass the gate


def test_sign_follows_the_readout_direction():
    est, rev = _clip(0.8, 7)[0], _clip(-0.8, 7)[0]
    print("r_hat", est[0], "reversed", rev[0])
    assert abs(rev[0] - (-0.8)) <= BOUND and abs(est[0] - 0.8) <= BOUND and rev[0] < 0.0 < est[0]


def test_end_to_end_the_estimate_recovers_what_the_true_value_would():
    est, _, motion, _ = _clip(0.8, 7)
    with_est, with_zero, with_true = (E.end_to_end(motion, ru, 0.8) for ru in (E.choose(est), 0.0, 0.8))
    print("r = 0.8: non-rigidity with the estimate %.4f, with 0 %.4f, with the true r %.4f" % (with_est, with_zero, with_true))
    assert with_est <= 1.15 * with_true and with_est <= 0.5 * with_zero
    est0, _, motion0, _ = _clip(0.0, 8)
    cost = E.end_to_end(motion0, E.choose(est0), 0.0) - E.end_to_end(motion0, 0.0, 0.0)
    print("r = 0: the estimate %.4f costs %.4f px" % (est0[0], cost))
    assert cost <= 0.05


def test_a_clip_without_information_is_refused():
    """A steady pan with no shake: constant velocity, so the regressor is measurement noise alone."""
    est = E.estimate_clip(E.rolling_clip(0.8, n=16, pose_fn=E.pan_pose))
    print("steady pan", est)
    assert est[1] > MAX_SE or not est[2] > 0.0
    assert E.choose(est, MAX_SE) == 0.0
    still = E.estimate_clip(np.repeat(E.rolling_clip(0.0, n=1), 8, 0))   # a tripod: no motion at all
    assert math.isnan(still[0]) and still[1] == math.inf and still[2] == 0.0 and E.choose(still) == 0.0
    assert E.choose(np.array([0.5, 0.01, 1.0, 100.0])) == 0.5 and E.choose(np.array([1.7, 0.01, 1.0, 100.0])) == 1.0
    assert E.choose(np.array([-1.7, 0.02, 1.0, 100.0])) == -1.0 and E.choose(np.array([0.5, 0.021, 1.0, 100.0])) == 0.0


def _terms(blocks, motion, cuts=None, order="forward"):
    return E.terms(*blocks, motion, S.shutter_rates(motion, cuts), S.SIZE, S.SIZE, scene_cuts=cuts, order=order)


def test_pairs_near_cuts_ends_and_nan_rows_are_zero():
    _, _, motion, blocks = _clip(0.8, 7)
    motion = np.array(motion)
    motion[25] = math.nan
    cuts = [10, 20]
    tm = _terms(blocks, motion, cuts)
    zero = {0, 1, 9, 10, 11, 19, 20, 21, 24, 25, 26, 31}   # within 2 of a cut or an end (the pair AT b - 1 has no pair ahead); next to NaN
    for k in range(S.N):
        assert (not tm[k].any()) == (k in zero), (k, tm[k])
        assert k in zero or tm[k, 3] >= E.MIN_BLOCKS
    assert np.array_equal(E.usable_pairs(motion, cuts), [k not in zero for k in range(S.N)])
    for T in range(4):   # fewer than 4 frames: no pair has a real pair on both sides
        short = E.terms(*(b[:T] for b in blocks), motion[:T], S.shutter_rates(motion[:T]), S.SIZE, S.SIZE)
        assert short.shape == (T, 4) and not short.any()
        est = E.estimate(short)
        assert math.isnan(est[0]) and est[1] == math.inf and est[2] == 0.0 and est[3] == 0.0
    # a pair with fewer than 8 valid blocks: a zero row, and its neighbours are untouched (their motion rows are inputs)
    act = np.array(blocks[2])
    act[5].reshape(-1)[7:] = 0
    few = _terms((blocks[0], blocks[1], act), np.array(_clip(0.8, 7)[2]))
    full = _clip(0.8, 7)[1]
    assert not few[5].any() and np.array_equal(np.delete(few, 5, 0), np.delete(full, 5, 0))


def test_cuts_do_not_leak():
    """Two scenes with opposite r, 16 frames each: the terms of the joined clip under the cut are those of each scene alone, bit for bit."""
    (_, _, ma, ba), (_, _, mb, bb) = _clip(0.8, 7), _clip(-0.8, 7)
    n = 16
    joined = tuple(np.concatenate([x[:n], y[:n]]) for x, y in zip(ba, bb))
    motion = np.concatenate([ma[:n], mb[:n]])
    tm = _terms(joined, motion, [n])
    alone_a, alone_b = _terms(tuple(x[:n] for x in ba), ma[:n]), _terms(tuple(y[:n] for y in bb), mb[:n])
    assert np.array_equal(tm[:n], alone_a) and np.array_equal(tm[n:], alone_b)
    ra, rb = E.estimate(alone_a)[0], E.estimate(alone_b)[0]
    print("scene estimates", ra, rb, "joined", E.estimate(tm)[0])
    assert ra > 0.5 and rb < -0.5
    # ... and without the cut the pairs on both sides of frame 16 would count
    assert _terms(joined, motion)[[n - 1, n + 1], 3].all() and not tm[n - 1:n + 2].any()


def test_summation_orders_agree():
    """The three orders -- forward, reverse, pairwise -- keep the same blocks and agree to 1e-10: the bound under which the GPU test's
    tolerance, 16 times this spread with a floor of 1e-12, stays far below anything the estimate means.  Reasoning: at most 196 blocks a
    pair, an epsilon of 2.2e-16, centred normal sums whose condition is a few hundred, terms of a few hundred at the most: 1e-13 .. 1e-12
    is what rounding can do, and 1e-10 leaves two decades."""
    _, _, motion, blocks = _clip(0.8, 7)
    margins = []
    rates = S.shutter_rates(motion)
    want = E.terms(*blocks, motion, rates, S.SIZE, S.SIZE, margins=margins)
    assert np.array_equal(want, _clip(0.8, 7)[1])
    spread, spread_est = 0.0, 0.0
    for order in ("reverse", "pairwise"):
        tm = E.terms(*blocks, motion, rates, S.SIZE, S.SIZE, order=order)
        assert np.array_equal(tm[:, 3], want[:, 3])
        spread = max(spread, float(np.abs(tm - want).max()))
        spread_est = max(spread_est, float(np.abs(E.estimate(tm, order)[:3] - E.estimate(want)[:3]).max()))
    print("spread of the terms", spread, "of the estimate", spread_est, "smallest inlier margin", min(margins))
    assert spread <= 1e-10 and spread_est <= 1e-10
