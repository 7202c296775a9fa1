"""CPU tests of the numpy restatement of the global-motion measurement (tests/motion_ref.py) and of stream.stability_scores' host
arithmetic: quantisation, planted integer shifts, the tie rule, an analytic texture on a planted path, and the scores on synthetic signals."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_ref as R  # noqa: E402


def test_quantisation_round_trip_and_special_values():
    k = np.arange(256)
    assert np.array_equal(R.quant(k.astype(np.float32) / np.float32(127.5) - np.float32(1)), k)
    v = np.array([np.nan, -np.nan, np.inf, -np.inf, -1.0, 1.0, -1.5, 1.5, -1e30, 1e30, 0.0, -0.0], np.float32)
    assert R.quant(v).tolist() == [0, 0, 255, 0, 0, 255, 0, 255, 0, 255, 128, 128]
    # a sample on a half rounds up, and contraction would not: at q + 0.5 exactly the three roundings land on the integer above
    k = np.arange(255, dtype=np.float32)
    on_half = ((k + np.float32(0.5)) - np.float32(0.5)) / np.float32(127.5) - np.float32(1)   # (v + 1) * 127.5 = k exactly where representable
    assert (np.abs(R.quant(on_half).astype(np.int64) - k.astype(np.int64)) <= 1).all()


def test_rank_is_the_lexicographic_order_of_length_then_dy_dx():
    """The kernel minimises (S, dx^2 + dy^2, dy, dx) lexicographically in place of S * 2048 + rank: the same candidate, since rank < 2048
    and rank sorts by exactly that triple."""
    for radius in (1, 4, 16):
        cand, rank = R.candidates(radius)
        assert sorted(rank.tolist()) == list(range((2 * radius + 1) ** 2)) and rank.max() <= 1088
        by_rank = [cand[i] for i in np.argsort(rank)]
        assert by_rank == sorted(cand, key=lambda c: (c[0] ** 2 + c[1] ** 2, c[0], c[1])) and by_rank[0] == (0, 0)


@pytest.mark.parametrize("radius,h,w", [(8, 64, 80), (16, 96, 80), (4, 40, 56)])
def test_planted_integer_shifts_are_found_exactly(radius, h, w):
    rs = np.random.RandomState(radius)
    m = radius - 1
    shifts = [(0, 0), (m, -m), (-m, m), (0, 0), (1, 0), (0, -1)] + [tuple(rs.randint(-m, m + 1, 2)) for _ in range(3)]
    planes = R.rolled_noise(shifts, h, w, seed=5)
    mv, sad, act = R.block_motion(planes, radius)
    nby, nbx = R.lattice(h, w, radius)
    assert mv.shape == (len(shifts), nby, nbx, 2) and not mv[0].any() and not sad[0].any()
    for t in range(1, len(shifts)):
        assert (mv[t] == np.array(shifts[t], np.int16)).all(), t
        assert (sad[t, ..., 0] == 0).all() and (sad[t, ..., 1:] > 0).all()
    assert (act > 20000).all()   # (uniform byte noise: 480 pairs of mean absolute difference 85)
    motion, inl = R.motion_fit(mv, sad, act, h, w, radius)
    assert motion[0].tolist() == [1.0, 0.0, 0.0, 0.0] and inl[0] == 0
    if nby * nbx >= R.MIN_BLOCKS:
        for t in range(1, len(shifts)):
            assert np.abs(motion[t] - np.array([1.0, 0.0, shifts[t][0], shifts[t][1]])).max() <= 1e-9, (t, motion[t])
            assert inl[t] == nby * nbx
    else:
        assert np.isnan(motion[1:]).all() and not inl.any()


def test_a_shift_of_exactly_the_radius_makes_the_pair_unfit():
    radius, h, w = 8, 64, 80
    shifts = [(0, 0), (radius, 0), (0, -radius), (-radius, radius), (radius - 1, radius - 1)]
    planes = R.rolled_noise(shifts, h, w, seed=9)
    mv, sad, act = R.block_motion(planes, radius)
    assert (mv[1] == (radius, 0)).all() and (mv[2] == (0, -radius)).all() and (sad[1, ..., 2] == -1).all() and (sad[2, ..., 3] == -1).all()
    assert (mv[3] == (-radius, radius)).all() and (sad[3, ..., 1] == -1).all() and (sad[3, ..., 4] == -1).all() and (sad[..., 0] == 0).all()
    motion, inl = R.motion_fit(mv, sad, act, h, w, radius)
    assert np.isnan(motion[1:4]).all() and not inl[1:4].any()
    assert np.abs(motion[4] - [1.0, 0.0, radius - 1, radius - 1]).max() <= 1e-9 and inl[4] == 12


def test_a_shift_beyond_the_radius_makes_the_pair_unfit():
    """A planted shift BEYOND the search range: the true match is outside the window, so every block of the noise plane takes the best of
    289 chance matches, which lies on the rim for only a few of them (radius 8, 12 blocks, shifts (11, 2) and (-9, -9): 10 and 12 of the 12
    vectors lie inside the rim, S at the best candidates 18 052 .. 19 936 against 0 for a true match).  What makes them invalid is the
    sharpness rule: around a chance match S is flat -- its two second differences together are 0.10 .. 0.41 of the activity on noise planes,
    against 0.95 .. 2.2 at the true matches of the texture, smooth and rolled clips -- and half the activity is asked for."""
    radius, h, w = 8, 64, 80
    shifts = [(0, 0), (radius + 3, 2), (-radius - 1, -radius - 1)]
    planes = R.rolled_noise(shifts, h, w, seed=9)
    mv, sad, act = R.block_motion(planes, radius)
    motion, inl = R.motion_fit(mv, sad, act, h, w, radius)
    inside = (np.abs(mv[1:].astype(np.int32)) < radius).all(-1).reshape(2, -1).sum(1)
    s = sad[1:].astype(np.int64)
    sharp = ((s[..., 1] + s[..., 2] - 2 * s[..., 0]) + (s[..., 3] + s[..., 4] - 2 * s[..., 0])) / act[1:]
    assert inside.min() >= 8 and sharp.max() < 0.5   # (the rim alone would leave enough blocks for a fit: the flat S rules them out)
    print("vectors inside the rim", inside.tolist(), "sharpness", sharp.min(), sharp.max(), "best S", sad[1:, ..., 0].min(), sad[1:, ..., 0].max(),
          "rows", motion[1:].tolist())
    assert np.isnan(motion[1:]).all() and not inl[1:].any()


def test_flat_plane_gets_zero_vectors_and_no_fit():
    planes = np.full((3, 64, 80), 0.25, np.float32)
    mv, sad, act = R.block_motion(planes, 8)
    assert not mv.any() and not sad.any() and not act.any()
    motion, inl = R.motion_fit(mv, sad, act, 64, 80, 8)
    assert np.isnan(motion[1:]).all() and not inl.any() and motion[0].tolist() == [1.0, 0.0, 0.0, 0.0]


@pytest.fixture(scope="module")
def texture_run():
    """64 frames of the analytic texture on the planted path, with and without jitter, and what the restatement measures on them"""
    out = {}
    for name, jitter, radius in (("jitter", True, 16), ("steady", False, 4)):   # (the steady pan moves 0.85 pixel a frame: a small search)
        poses = R.planted_path(64, seed=11, jitter=jitter)
        planes = R.texture_clip(poses, 256, 256, seed=3)
        mv, sad, act = R.block_motion(planes, radius)
        margins = []
        motion, inl = R.motion_fit(mv, sad, act, 256, 256, radius, margins=margins)
        out[name] = (poses, motion, inl, act, margins)
    return out


def test_analytic_texture_on_a_planted_path_is_recovered(texture_run):
    """Bounds from the issue's prototype of the same definition (0.053 deg, 0.115 pixel measured there; about twice that allowed).  This
    restatement measures 0.085 deg and 0.227 pixel on its own texture and path with the jitter (seeds 3 and 11; pairs that turn by up to
    1.2 deg, which a 16 x 16 block match only follows in part) and 0.013 deg and 0.083 pixel without: inside the bounds, above the prototype's."""
    for name in ("jitter", "steady"):
        poses, motion, inl, act, _ = texture_run[name]
        want = R.expected_motion(poses)
        assert np.isfinite(motion).all() and (inl[1:] >= 100).all(), name
        rot = np.rad2deg(np.abs(np.arctan2(motion[1:, 1], motion[1:, 0]) - want[1:, 0])).max()
        tr = np.abs(motion[1:, 2:] - want[1:, 1:]).max()
        print(name, "rotation error [deg]", rot, "translation error [px]", tr, "activity", act.min(), act.max(), "inliers", inl[1:].min())
        assert rot <= 0.1 and tr <= 0.25, (name, rot, tr)
        assert act.min() >= 2000   # (the default min_activity keeps every block of this texture)


def test_no_block_lies_on_a_round_threshold(texture_run):
    """The condition under which the GPU test may ask for equal inlier counts: no valid block's squared residual within a relative 1e-3
    of a round's threshold (the last bits of a residual then cannot flip an inlier)."""
    for name in ("jitter", "steady"):
        margins = texture_run[name][4]
        print(name, "smallest margin", min(margins))
        assert min(margins) > 1e-3


def test_stability_scores_on_synthetic_signals(texture_run):
    from pwstablenet_amd.stream import stability_scores
    steady = stability_scores(texture_run["steady"][1])
    shaky = stability_scores(texture_run["jitter"][1])
    print("steady", steady["scenes"][0], "shaky", shaky["scenes"][0])
    for got, want in ((steady, R.stability_scores(texture_run["steady"][1])), (shaky, R.stability_scores(texture_run["jitter"][1]))):
        assert got == want
    m = texture_run["steady"][1]
    for sig in (m[:, 2], m[:, 3], np.arctan2(m[:, 1], m[:, 0])):
        assert R.signal_score(sig) >= 0.95
    m = texture_run["jitter"][1]
    for sig in (m[:, 2], m[:, 3], np.arctan2(m[:, 1], m[:, 0])):
        assert R.signal_score(sig) <= 0.6
    assert steady["stability"] >= 0.95 and shaky["stability"] <= 0.6 and len(steady["scenes"]) == 1
    assert steady["stability"] == min(steady["translation"], steady["rotation"])


def _motion_rows(tx, ty=None, th=None):
    n = len(tx)
    ty = np.zeros(n) if ty is None else ty
    th = np.zeros(n) if th is None else th
    return np.stack([np.cos(th), np.sin(th), tx, ty], 1)


def test_stability_scores_rules():
    from pwstablenet_amd.stream import stability_scores
    k = np.arange(64, dtype=np.float64)
    # a "walk": the path sways slowly (one and a half periods over the scene), no jitter -- its velocity is the path's difference
    path = 6.0 * np.sin(2 * np.pi * 1.5 * k / 64)
    walk = _motion_rows(np.diff(path, prepend=0.0), np.diff(0.5 * path, prepend=0.0), np.deg2rad(np.diff(0.2 * path, prepend=0.0)))
    s = stability_scores(walk)
    assert s["translation"] >= 0.99 and s["rotation"] >= 0.99 and s["stability"] >= 0.99
    assert s == R.stability_scores(walk)
    still = _motion_rows(np.zeros(40))
    assert stability_scores(still)["stability"] == 1.0 and stability_scores(still)["scenes"][0]["rotation"] == 1.0
    assert math.isnan(stability_scores(_motion_rows(np.zeros(23)))["stability"])
    assert stability_scores(_motion_rows(np.zeros(24)))["stability"] == 1.0
    holed = walk.copy()
    holed[30] = np.nan
    assert math.isnan(stability_scores(holed)["stability"]) and math.isnan(stability_scores(holed)["scenes"][0]["translation"])
    # cuts split the signals: the pair at the cut belongs to neither scene, so a NaN (or a jump) there changes nothing
    rs = np.random.RandomState(2)
    jit = [np.diff(rs.normal(0, sd, 32), prepend=0.0) for sd in (2.0, 2.0, np.deg2rad(0.3))]   # pose jitter: the pairs are its differences
    two = np.concatenate([walk[:32], _motion_rows(*jit)])
    two[32] = np.nan
    s2 = stability_scores(two, scene_cuts=[32])
    assert [(c["start"], c["end"]) for c in s2["scenes"]] == [(0, 32), (32, 64)]
    assert s2["scenes"][0]["stability"] == stability_scores(walk[:32])["stability"]
    assert s2["scenes"][1]["stability"] < 0.7 < s2["scenes"][0]["stability"]
    assert abs(s2["stability"] - 0.5 * (s2["scenes"][0]["stability"] + s2["scenes"][1]["stability"])) < 1e-15
    assert math.isnan(stability_scores(two)["stability"])                                     # without the cut the NaN pair counts
    short = stability_scores(two[:50], scene_cuts=[32])                                         # a scene of 18 frames has no score ...
    assert math.isnan(short["scenes"][1]["stability"]) and short["stability"] == short["scenes"][0]["stability"]   # ... and no weight
    assert s2 == R.stability_scores(two, [32])
    with pytest.raises(ValueError):
        stability_scores(np.zeros((10, 3)))
    with pytest.raises(ValueError):
        stability_scores(walk, scene_cuts=[64])
    import torch
    assert stability_scores(torch.from_numpy(walk))["stability"] == s["stability"]
