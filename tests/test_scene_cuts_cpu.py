"""CPU tests of the scene-cut support: the cut rule, the per-scene crop recurrence, the restated score on synthetic joins (the condition
the GPU test of scene_cuts="auto" rests on), the per-scene window table and the C ABI entry."""
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_ref as R  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_PAIRS = [(1, 2), (3, 4), (5, 6), (123, 321), (7, 8), (9, 10)]


def test_find_scene_cuts_rule():
    from pwstablenet_amd.stream import find_scene_cuts
    s = [0.0] * 64
    s[20] = 0.25                       # the threshold is strict
    assert find_scene_cuts(s) == []
    s[20] = 0.2500001
    assert find_scene_cuts(s) == [20]
    assert find_scene_cuts(s, threshold=0.3) == []
    # min_scene counts from frame 0 ...
    s = [0.0] * 64
    s[15] = s[16] = 0.9
    assert find_scene_cuts(s) == [16]
    assert find_scene_cuts(s, min_scene=15) == [15]            # (16 is then one frame after an accepted cut)
    assert find_scene_cuts(s, min_scene=1) == [15, 16]
    # ... and from the last ACCEPTED cut: a dropped candidate does not restart the count
    s = [0.0] * 64
    s[20] = s[30] = s[36] = s[51] = s[52] = 0.9
    assert find_scene_cuts(s) == [20, 36, 52]                  # 30 dropped (10 after 20); 36 = 20 + 16 stands although 30 came between
    s[0] = 5.0                                                 # frame 0 starts the clip, never a cut
    assert find_scene_cuts(s) == [20, 36, 52]
    assert find_scene_cuts([]) == [] and find_scene_cuts([0.9]) == []
    assert find_scene_cuts(torch.zeros(0)) == [] and find_scene_cuts(np.ones(1)) == []
    # one result for a tensor, a list and an array -- and the restatement's
    rs = np.random.RandomState(0)
    v = (rs.rand(300) * 0.5).astype(np.float32)
    want = R.find_cuts(v)
    assert len(want) > 3
    assert find_scene_cuts(torch.from_numpy(v)) == find_scene_cuts(v.tolist()) == find_scene_cuts(v) == want
    assert find_scene_cuts(v, 0.4, 5) == R.find_cuts(v, 0.4, 5)
    # causal: a prefix gives the prefix of the result
    assert find_scene_cuts(v[:150]) == [c for c in want if c < 150]


def test_auto_crop_window_per_scene():
    from pwstablenet_amd.stream import auto_crop_window
    rs = np.random.RandomState(3)
    T, hw = 80, (360, 640)
    b = np.stack([rs.uniform(0, 40, T), rs.uniform(320, 360, T), rs.uniform(0, 60, T), rs.uniform(580, 640, T)], 1)
    want = auto_crop_window(b, hw, (180, 320))
    assert auto_crop_window(b, hw, (180, 320), scene_cuts=None) == want
    assert auto_crop_window(b, hw, (180, 320), scene_cuts=[]) == want
    assert auto_crop_window(torch.from_numpy(b), hw, (180, 320), 30, scene_cuts=[]) == want
    # with a cut at c the frames c - 15 .. c + 15 are not read (they see a clamped window, as the clip's ends do): the window is that
    # of the recurrence run over the two ranges in turn
    c = 40
    cut = auto_crop_window(b, hw, scene_cuts=[c])
    x0, x1, y0, y1 = 0.0, 640.0, 0.0, 360.0
    for i in list(range(16, c - 15)) + list(range(c + 16, T - 15)):
        top, bottom, left, right = b[i]
        y0 += (top - y0) * 0.5 if y0 < top else 0.0
        y1 -= (y1 - bottom) * 0.5 if y1 > bottom else 0.0
        x0 += (left - x0) * 0.5 if x0 < left else 0.0
        x1 -= (x1 - right) * 0.5 if x1 > right else 0.0
    assert cut == (x0, x1, y0, y1)
    assert cut != auto_crop_window(b, hw)
    nan = b.copy()
    nan[c - 15:c + 16] = np.nan
    assert auto_crop_window(nan, hw, scene_cuts=[c]) == cut           # not read: no error
    with pytest.raises(ValueError, match="frame 25"):
        auto_crop_window(nan, hw)                                      # without the cut they are
    for i in (16, c - 16, c + 16, T - 16):                             # the first / last frame read of either scene
        bad = b.copy()
        bad[i] = np.nan
        with pytest.raises(ValueError, match="frame %d " % i):
            auto_crop_window(bad, hw, scene_cuts=[c])
    with pytest.raises(ValueError):
        auto_crop_window(b, hw, scene_cuts=[50, 40])
    with pytest.raises(ValueError):
        auto_crop_window(b, hw, scene_cuts=[T])


@pytest.fixture(scope="module")
def joined_scores():
    """restated scores of the six 40-frame clips made of two 20-frame synthetic scenes"""
    return [R.scores(np.concatenate([synth.make_window(1, 20, 256, a)[0], synth.make_window(1, 20, 256, b)[0]])) for a, b in SEED_PAIRS]


def test_default_threshold_separates_synthetic_joins(joined_scores):
    """What 0.25 rests on (INTEGRATION.md "Scene cuts"): within a shaky synthetic scene every score stays at or below the threshold, at a
    join of two scenes it lies above.  The restatement alone: the GPU test of scene_cuts="auto" depends on this condition."""
    from pwstablenet_amd.stream import find_scene_cuts
    within, joins = [], []
    for sc in joined_scores:
        assert sc.dtype == np.float32 and sc.shape == (40,) and sc[0] == 0
        assert np.all(np.delete(sc, 20) <= 0.25), float(np.delete(sc, 20).max())
        assert sc[20] > 0.25, float(sc[20])
        assert R.find_cuts(sc) == [20] and find_scene_cuts(sc) == [20]
        within.append(np.delete(sc, [0, 20]))
        joins.append(float(sc[20]))
    within = np.concatenate(within)
    print("within-scene max %.3f mean %.3f; joins %.3f .. %.3f" % (within.max(), within.mean(), min(joins), max(joins)))
    assert within.max() < 0.15 and min(joins) > 0.3          # the figures INTEGRATION.md quotes: 0.123 and 0.351


def test_bins_at_the_edges():
    e = (np.arange(33, dtype=np.float32) / np.float32(16) - np.float32(1)).astype(np.float32)
    assert R.bins(e).tolist() == list(range(32)) + [31]
    lo, hi = np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))
    # a neighbour of an edge: v + 1 is ROUNDED to fp32 first (near 0 the neighbours are finer than fp32 resolves at 1, and v + 1 lands on the
    # edge again); expected from float64, where the sum is exact, rounded once
    def want(v):
        x = np.float32(np.float64(v) + 1.0).astype(np.float64) * 16.0
        return np.clip(np.floor(x), 0, 31).astype(int).tolist()
    assert R.bins(lo).tolist() == want(lo) and R.bins(hi).tolist() == want(hi)
    assert R.bins(lo)[:9].tolist() == [0] + list(range(8))     # in [-1, -0.5] the sum is exact: just below edge k is bin k - 1 (below -1: bin 0)
    assert R.bins(lo)[17:].tolist() == list(range(17, 32)) + [31] and R.bins(hi).tolist() == list(range(32)) + [31]
    assert R.bins(np.array([np.nan, -np.inf, np.inf, -1.0, 1.0, -5.0, 5.0], np.float32)).tolist() == [0, 0, 31, 0, 31, 0, 31]


def test_windows_index_one_scene_is_the_reference_clamp():
    for T in (1, 7, 31, 40):
        tab = R.windows_index(T, [])
        for i in range(T):
            want = torch.clamp(torch.arange(i - 15, i + 16), 0, T - 1)       # tests/test_hip_stream.py::per_frame_reference
            assert tab[i].tolist() == want.tolist()
    tab = R.windows_index(40, [21])
    assert tab[20].tolist() == list(range(5, 21)) + [20] * 15 and tab[21].tolist() == [21] * 15 + list(range(21, 37))


@pytest.mark.parametrize("T,hl,hr,cuts,batch", [(34, 0, 0, [21], 4), (40, 0, 0, [5, 26], 4), (30, 3, 2, [2, 20], 4), (30, 3, 2, [17, 34], 8),
                                                 (50, 15, 15, [10, 40, 70], 8), (9, 0, 0, [], 4), (20, 15, 0, [15], 32), (12, 0, 0, [1, 2, 11], 5)])
def test_layout_windows_equal_the_index_table(T, hl, hr, cuts, batch):
    """VideoStabilizer._layout on the host: the strided windows of the padded buffer hold exactly the planes of the clamped index table,
    every frame belongs to one batch, and no batch spans a cut."""
    from pwstablenet_amd.stream import VideoStabilizer, _windows
    n = T + hl + hr
    gray = torch.arange(n, dtype=torch.float32).view(n, 1, 1).expand(n, 4, 4).contiguous()
    vs = VideoStabilizer(None, batch=batch, device="cpu")
    gp, batches = vs._layout(gray, hl, hr, T, cuts)
    tab = R.windows_index(n, cuts)
    seen = []
    edges = [0] + cuts + [n]
    for s, e, start in batches:
        assert 0 < e - s <= batch
        win = _windows(gp, start, e - s, 30)
        assert win.shape == (e - s, 31, 4, 4)
        for k in range(e - s):
            assert win[k, :, 0, 0].long().tolist() == tab[hl + s + k].tolist(), (s, k)
        assert sum(a <= hl + s < b and hl + e <= b for a, b in zip(edges[:-1], edges[1:])) == 1      # inside one scene
        seen += list(range(s, e))
    assert seen == list(range(T))
    # batches restart at every scene's first frame to stabilise
    starts = {max(a, hl) - hl for a, b in zip(edges[:-1], edges[1:]) if max(a, hl) < min(b, hl + T)}
    assert starts <= {s for s, _, _ in batches}


def test_run_refuses_bad_cut_lists_before_touching_the_device():
    from pwstablenet_amd.stream import _check_cuts
    assert _check_cuts([3, 9], 10, "x") == [3, 9] and _check_cuts(torch.tensor([4]), 10, "x") == [4] and _check_cuts((), 10, "x") == []
    for bad in ([0], [10], [5, 5], [6, 5], [-1], ["a"], 3):
        with pytest.raises(ValueError):
            _check_cuts(bad, 10, "x")


def test_abi_declares_pws_scene_change():
    from pwstablenet_amd import build, hipabi
    hdr = open(os.path.join(ROOT, "include", "pwstable.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int pws_scene_change\(const float \*planes, int n, int h, int w, unsigned \*hist, unsigned \*sad, "
                  r"pws_stream_t stream\);", hdr, re.S)
    assert m and "main_new.py:627-633" in m.group(1)
    res, args = hipabi.SIGNATURES["pws_scene_change"]
    assert res is hipabi._I and len(args) == 7
    assert "scene.hip" in build.SOURCES
    assert hipabi.ABI_VERSION == 5
