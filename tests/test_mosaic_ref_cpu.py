"""CPU tests of tests/mosaic_ref.py, the float64 restatement the GPU tests of the "mosaic" borders are held to: the rule on hand-made coverage
arrays (no fields), the packing of the eleven formats, and the condition on the GPU tests' fields -- at most keep_ref.CAP (1 %) of a case's
samples undecided, a sample being undecided if any frame within +-R of it has the position within delta = keep_ref.FACTOR x the plane's
fp32 coordinate error of a coverage threshold."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keep_ref as K  # noqa: E402
import mosaic_ref as M  # noqa: E402


def column(bits):
    """A clip of one-position frames from a string of 0 / 1: (T, 1) coverage, and frames whose only sample is 10 (t + 1)."""
    cov = np.array([[c == "1"] for c in bits])
    return (10 * (np.arange(len(bits)) + 1)).astype(np.uint8)[:, None], cov


def test_past_wins_a_tie():
    w, cov = column("101")
    out, d = M.mosaic(w, cov, 3)
    assert d[:, 0].tolist() == [0, -1, 0] and out[:, 0].tolist() == [10, 10, 30]


def test_the_nearer_frame_wins_over_the_earlier_one():
    w, cov = column("10010")
    out, d = M.mosaic(w, cov, 3)
    assert d[:, 0].tolist() == [0, -1, 1, 0, -1] and out[:, 0].tolist() == [10, 10, 40, 40, 40]


def test_the_search_stops_at_the_radius_and_at_both_ends_of_the_scene():
    w, cov = column("1000000001")
    out, d = M.mosaic(w, cov, 3)
    assert d[:, 0].tolist() == [0, -1, -2, -3, M.NONE, M.NONE, 3, 2, 1, 0]
    assert out[:, 0].tolist() == [10, 10, 10, 10, 50, 60, 100, 100, 100, 100]   # (no donor: the warp's own sample stays)
    assert M.unfilled(cov, 3).tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    w, cov = column("0001000")   # the ends of the scene: nothing before frame 0 or after frame n-1 is looked at
    out, d = M.mosaic(w, cov, 2)
    assert d[:, 0].tolist() == [M.NONE, 2, 1, 0, -1, -2, M.NONE] and out[:, 0].tolist() == [10, 40, 40, 40, 40, 40, 70]
    out, d = M.mosaic(*column("000"), 15)
    assert (d == M.NONE).all() and out[:, 0].tolist() == [10, 20, 30]
    assert M.mosaic(*column("0001000"), 1)[1][:, 0].tolist() == [M.NONE, M.NONE, 1, 0, -1, M.NONE, M.NONE]


def random_clip(seed, t=12, shape=(5, 7), p=0.45):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (t,) + shape).astype(np.uint8), rs.rand(t, *shape) < p


def test_unfilled_counts_and_covered_samples():
    w, cov = random_clip(0)
    for r in (1, 3, 15):
        out, d = M.mosaic(w, cov, r)
        assert np.array_equal(out[cov], w[cov]) and (d[cov] == 0).all() and (d[~cov] != 0).all()
        assert np.array_equal(out[d == M.NONE], w[d == M.NONE])
        assert np.array_equal(M.unfilled(cov, r), (d == M.NONE).reshape(len(w), -1).sum(1))
        for t in range(len(w)):   # every sample is a copy of the sample its distance names, and that donor is covered there
            for k in np.unique(d[t]):
                if k not in (0, M.NONE):
                    sel = d[t] == k
                    assert abs(k) <= r and cov[t + k][sel].all() and np.array_equal(out[t][sel], w[t + k][sel])
                    near = [o for j in range(1, abs(k)) for o in (-j, j)] + ([-k] if k > 0 else [])
                    assert not any(cov[t + o][sel].any() for o in near if 0 <= t + o < len(w))   # (nothing nearer; no past frame as near)
    assert M.unfilled(cov, 1).sum() > M.unfilled(cov, 3).sum() > 0


@pytest.mark.parametrize("cuts", [(0, 12), (0, 4, 12), (0, 1, 2, 7, 12), (0, 5, 6, 12)])
def test_any_chunking_equals_the_whole_clip(cuts):
    """Filling [start, stop) chunk by chunk, in either order, with frames that have been filled as donors, gives the whole-clip result."""
    w, cov = random_clip(1)
    want, _ = M.mosaic(w, cov, 3)
    for order in (1, -1):
        buf = w.copy()
        for a, b in list(zip(cuts[:-1], cuts[1:]))[::order]:
            before = buf.copy()
            M.fill_range_(buf, cov, 3, a, b)
            assert np.array_equal(buf[:a], before[:a]) and np.array_equal(buf[b:], before[b:])
            assert np.array_equal(buf[a:b], want[a:b])
        assert np.array_equal(buf, want)


def test_packing_of_the_eleven_formats():
    assert len(M.FORMATS) == 11
    t, h, w = 2, 4, 8
    for fmt, (dt, inter, sh) in M.FORMATS.items():
        sizes = M.plane_sizes(fmt, h, w)
        y = np.full((t, h, w), 1)
        c = np.full((t,) + sizes[-1], 2) + np.arange(sizes[-1][1])   # (chroma values 2 + column)
        p = M.packed(y, c, fmt)
        assert p.shape == M.frame_shape(fmt, t, h, w), fmt
        if fmt == "bgr24":
            assert (p == 1).all()
            continue
        assert (p[:, :h] == 1).all() and sizes[1] == (h >> sh[1], w >> sh[0])
        ch, cw = sizes[1]
        flat = p[:, h:].reshape(t, -1)
        if inter:
            assert np.array_equal(flat.reshape(t, ch, cw, 2)[..., 0], c) and np.array_equal(flat.reshape(t, ch, cw, 2)[..., 1], c)
        else:
            assert np.array_equal(flat.reshape(t, 2, ch, cw)[:, 0], c) and np.array_equal(flat.reshape(t, 2, ch, cw)[:, 1], c)
    assert M.frame_shape("nv12", 1, 16, 20) == (1, 24, 20) and M.frame_shape("i422", 1, 16, 20) == (1, 32, 20) and M.frame_shape("i410", 1, 16, 20) == (1, 48, 20)


def test_undecided_spreads_over_the_radius():
    dist = np.ones((9, 1, 2))
    dist[4, 0, 0] = 0.0
    u = M.undecided(dist, 0.5, 3)
    assert u[:, 0, 0].tolist() == [False] + [True] * 7 + [False] and not u[:, 0, 1].any()


def plane_sizes_of(h, w):
    """Every plane size the eleven formats give an h x w frame."""
    return sorted({s for fmt in M.FORMATS for s in M.plane_sizes(fmt, h, w)})


def gpu_cases():
    for h, w, fs in M.SHAPES:
        for case in M.FIELDS:
            yield h, w, fs, case
    yield M.BIG + ("ramp",)
    yield M.BIG + ("smooth",)


@pytest.mark.parametrize("h,w,fs,case", list(gpu_cases()))
def test_condition_on_the_gpu_fields(h, w, fs, case):
    """Every field tests/test_hip_mosaic.py uses leaves at most 1 % of each plane's samples undecided, by the restatement alone; on "ramp"
    every donor distance -R .. R occurs in every plane, and so does "unfilled" except on the small shapes under align_corners=True with the
    bilinear margin (see below), where exactly that is asserted."""
    field = M.field_case(case, fs, seed=w)
    assert field.shape == (M.T, fs, fs, 2) and field.dtype == np.float32
    for ac in (False, True):
        for ph, pw in plane_sizes_of(h, w):
            delta = K.FACTOR * K.fp32_error(field, ph, pw, ac)
            assert delta < 1e-2, delta
            for m in (0, 1):
                cov, dist = K.coverage(field, ph, pw, ac, m)
                share = float(M.undecided(dist, delta, M.R).mean())
                d = M.donors(cov, M.R)
                print("%dx%d %s ac=%d m=%d: delta %.3g, undecided %.5f, uncovered %.3f, unfilled %.3f" % (ph, pw, case, ac, m, delta, share, 1 - cov.mean(),
                                                                                                     (d == M.NONE).mean()))
                assert share <= K.CAP, share
                if case == "identity":
                    assert cov.all() or m == 1
                elif case == "ramp":
                    # The 8 x 8 field spans +-0.875: with align_corners=True it draws every plane in by 6 % on each side, the bilinear margin
                    # then leaves only the three frames at either end with a wedge, and frame 3 covers frame 0's: no position there is
                    # without a donor within 3.  (The bicubic margin, align_corners=False and the 720p case all have some.)
                    no_none = fs == 8 and ac and m == 0
                    want = set(range(-M.R, M.R + 1)) | (set() if no_none else {M.NONE})
                    assert set(np.unique(d).tolist()) == want, (ph, pw, ac, m, np.unique(d).tolist())
                else:
                    assert not cov.all() and cov.any() and (d == M.NONE).any()
