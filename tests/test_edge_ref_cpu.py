"""CPU tests of tests/edge_ref.py, the float64 restatement the GPU tests of the edge modes are held to: ``fold``'s properties; agreement of
the folded-tap rule with torch's own padding modes (``grid_sample(padding_mode="border" | "reflection", align_corners=True)`` on pixel
coordinates, both interpolations); the condition on the GPU test's fields -- at most keep_ref.CAP (1 %) of a plane's positions undecided,
i.e. within delta = keep_ref.FACTOR x the plane's fp32 coordinate error of a coverage threshold; and the acceptance itself: the restatement
evaluated in numpy float32 on keep_ref.coordinates32 -- what a correct fp32 kernel computes, up to the order of its operations -- passes
edge_ref.check_case against float64 on every input of tests/test_hip_edge.py, 720p included, and the shares it leaves are printed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as E  # noqa: E402
import keep_ref as K  # noqa: E402


@pytest.fixture(autouse=True, scope="module")
def the_modes_are_the_packages():
    """What is restated here are the package's modes: functional.EDGES names "pad" (no pass) and then exactly edge_ref.EDGES, in the order of
    the C entries' ``edge`` argument (1 clamp, 2 mirror); the interpolations are the package's too."""
    pytest.importorskip("torch")
    from pwstablenet_amd import functional as PF
    assert PF.EDGES == ("pad",) + tuple(E.EDGES) and tuple(PF.INTERPOLATIONS) == tuple(E.MODES)


def test_fold_is_the_identity_inside_the_plane():
    for n in (1, 2, 5, 720):
        i = np.arange(n)
        for edge in E.EDGES:
            assert np.array_equal(E.fold(i, n, edge), i)


def test_fold_clamp():
    assert E.fold([-7, -1, 0, 3, 4, 5, 1 << 40, -(1 << 40)], 5, "clamp").tolist() == [0, 0, 0, 3, 4, 4, 4, 0]
    assert E.fold([-3, 0, 9], 1, "clamp").tolist() == [0, 0, 0]


def test_fold_mirror_reflects_without_repeating_the_edge():
    # n = 5: ... 2 1 | 0 1 2 3 4 | 3 2 1 0 1 ...
    assert E.fold(np.arange(-6, 14), 5, "mirror").tolist() == [2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3]
    assert E.fold(np.arange(-4, 5), 2, "mirror").tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0]
    assert E.fold([-5, -1, 0, 1, 77, -(1 << 40)], 1, "mirror").tolist() == [0] * 6


def test_fold_mirror_has_period_2n_minus_2_and_is_even():
    rs = np.random.RandomState(0)
    for n in (2, 3, 10, 641):
        i = rs.randint(-10 ** 9, 10 ** 9, 1000)
        f = E.fold(i, n, "mirror")
        assert ((0 <= f) & (f < n)).all()
        assert np.array_equal(f, E.fold(i + 2 * (n - 1), n, "mirror")) and np.array_equal(f, E.fold(i - 14 * (n - 1), n, "mirror"))
        assert np.array_equal(f, E.fold(-i, n, "mirror"))   # reflection about sample 0
        assert np.array_equal(f, E.fold(2 * (n - 1) - i, n, "mirror"))   # and about sample n - 1
    with pytest.raises(ValueError):
        E.fold([0], 4, "wrap")


def test_equal_taps_give_their_value_exactly():
    rs = np.random.RandomState(1)
    ix, iy = rs.uniform(-40, 60, (2, 9, 12)), rs.uniform(-40, 60, (2, 9, 12))
    for v in (0, 37, 255, 1023):
        plane = np.full((2, 9, 12), v)
        for edge in E.EDGES:
            for mode in E.MODES:
                for dt in (np.float64, np.float32):
                    assert (E.sample_plane(plane, ix.astype(dt), iy.astype(dt), edge, mode, dtype=dt) == v).all()


@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("edge", E.EDGES)
def test_agrees_with_torch_padding_modes(edge, mode):
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    rs = np.random.RandomState(5)
    worst = 0.0
    for h, w in ((7, 9), (16, 20), (1, 6), (33, 2)):
        plane = rs.uniform(0, 255, (3, h, w, 2))
        ix = rs.uniform(-2.8 * w, 3.8 * w, (3, 11, 13))
        iy = rs.uniform(-2.8 * h, 3.8 * h, (3, 11, 13))
        ix[0, 0, :4], iy[0, 0, :4] = [0.0, w - 1.0, -1.0, 2.0 * w], [0.0, h - 1.0, h + 0.5, -3.0]   # on the samples and on the rim
        got = E.sample_plane(plane, ix, iy, edge, mode).reshape(3, 11, 13, 2)
        # pixel coordinates under align_corners=True: g = 2 i / (n - 1) - 1 (an axis of one sample reads that sample wherever it is asked)
        gx = 2 * ix / (w - 1) - 1 if w > 1 else np.zeros_like(ix)
        gy = 2 * iy / (h - 1) - 1 if h > 1 else np.zeros_like(iy)
        if mode == "bicubic" and (h == 1 or w == 1):
            continue   # (torch's bicubic taps of a one-sample axis are not all that sample: its coordinates there are degenerate)
        want = F.grid_sample(torch.from_numpy(plane).permute(0, 3, 1, 2), torch.from_numpy(np.stack([gx, gy], -1)), mode=mode,
                             padding_mode={"clamp": "border", "mirror": "reflection"}[edge], align_corners=True).permute(0, 2, 3, 1).numpy()
        worst = max(worst, float(np.abs(got - want).max()))
    print("%s %s: largest distance from torch %.3g" % (edge, mode, worst))
    assert worst < 1e-9


def test_the_fields_leave_few_positions_undecided():
    worst = 0.0
    sizes = set()
    for h, w, fs in E.SHAPES:
        sizes |= {(h, w, fs, w), (h // 2, w // 2, fs, w), (h, w // 2, fs, w)}   # Y / 4:4:4 chroma, 4:2:0 chroma, 4:2:2 chroma
    for ph, pw, fs, seed in sorted(sizes):
        for case in E.FIELDS:
            for ac in (False, True):
                field = E.field_of(case, fs, seed)
                delta = K.FACTOR * K.fp32_error(field, ph, pw, ac)
                for m in (0, 1):
                    share = float((K.coverage(field, ph, pw, ac, m)[1] <= delta).mean())
                    assert share <= K.CAP, (ph, pw, case, ac, m, share)
                    worst = max(worst, share)
    print("largest share of undecided positions on the small shapes: %.5f" % worst)


def run32(fmt_name, h, w, fs, case, ac, mode, edge):
    _, _, refs = E.case_reference(fmt_name, h, w, fs, case, ac, mode, edge, float32=True)
    warped = E.warped_of(fmt_name, h, w)
    got = E.restated32(warped, refs, fmt_name)
    return E.check_case(got, warped, refs, fmt_name, (fmt_name, h, w, case, ac, mode, edge), E.compares(case, edge))


@pytest.mark.parametrize("fmt_name", E.FORMATS)
def test_float32_restatement_passes_the_gpu_tests_acceptance(fmt_name):
    worst, und = 0.0, 0.0
    for h, w, fs in E.SHAPES:
        for case, ac, mode, edge in E.small_cases():
            share, u = run32(fmt_name, h, w, fs, case, ac, mode, edge)
            worst, und = max(worst, share), max(und, u)
    print("%s small shapes: largest share of differing uncovered samples %.5f, of undecided positions %.5f" % (fmt_name, worst, und))
    h, w, fs = E.BIG
    case, ac, mode, edge = E.BIG_CASE[fmt_name]
    share, u = run32(fmt_name, h, w, fs, case, ac, mode, edge)
    print("%s 720p %s ac=%s %s %s: share of differing uncovered samples %.5f, of undecided positions %.5f" % (fmt_name, case, ac, mode, edge, share, u))


def test_fill_is_the_rule_on_whole_frames():
    """edge_ref.fill on a hand-checkable case: 1-row shift to the left by 2 samples (align_corners=True, bilinear), Y of an i444 frame."""
    h, w = 4, 8
    src = (np.arange(3 * h * w).reshape(1, 3 * h, w) % 251).astype(np.uint8)
    warped = np.full_like(src, 7)
    xs, ys = np.meshgrid(np.linspace(-1, 1, w) + 2 * 2 / (w - 1), np.linspace(-1, 1, h), indexing="xy")   # ix = x + 2, iy = y
    field = np.stack([xs, ys], -1)[None].astype(np.float64)
    y = src[0, :h].astype(np.int64)
    for edge, cols in (("clamp", [2, 3, 4, 5, 6, 7, 7, 7]), ("mirror", [2, 3, 4, 5, 6, 7, 6, 5])):
        out = E.fill(warped, src, field, "i444", edge, "bilinear", True)
        want = y[:, cols]
        want[:, :6] = 7   # covered (ix <= w - 1): the warp's bytes stay
        got = out[0, :h].astype(np.int64)
        # float64 coordinates of a linspace field may sit a rounding off the integers: the uncovered columns are checked to 1 LSB, the rest exactly
        assert np.array_equal(got[:, :5], want[:, :5]) and np.abs(got[:, 6:] - want[:, 6:]).max() <= 1, (edge, got, want)


def test_edge_entries_are_declared():
    pytest.importorskip("torch")
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import hipabi
    assert PF.EDGES == ("pad", "clamp", "mirror")
    names = set()
    for name in list(PF.FRAME_FORMATS) + list(PF.CHROMA_FORMATS):
        entry = PF.lookup_format(name).edge_entry
        assert entry in hipabi.SIGNATURES, (name, entry)
        names.add(entry)
    assert names == {"pws_border_edge_u8", "pws_border_edge_yuv_u8", "pws_border_edge_yuv_u16"}
    assert len(hipabi.SIGNATURES["pws_border_edge_u8"][1]) == 13 and len(hipabi.SIGNATURES["pws_border_edge_yuv_u8"][1]) == 14
