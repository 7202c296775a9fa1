"""Deblurring without a GPU: the float64 / integer restatement (tests/deblur_ref.py) pinned on a clip with one blurred frame -- the blurred
frame's sharpness is a fraction of its neighbours', they lend it detail, its error against the clean clip falls and its sharpness rises --
the plan's stopping rules, and every argument check of the feature.  The figures asserted are margins around what this restatement
measures on this clip (INTEGRATION.md quotes them): 7 frames of 96 x 64, a texture translating by (1.25, 0.5) pixel a frame, frame 3 blurred
by a 5-tap horizontal box, R = 2."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(1, ROOT)

import deblur_ref as D  # noqa: E402

N, H, W, R, BLURRED = 7, 64, 96, 2, 3


@pytest.fixture(scope="module")
def clips():
    clip, clean = D.texture(N, H, W, 11, blurred=(BLURRED,))
    return {fmt: (D.to_format(clip, fmt, 1), D.to_format(clean, fmt, 1)) for fmt in ("bgr24", "nv12", "p010")}


def _mae(a, b, fmt):
    return float(np.abs(D.samples(a, fmt)[BLURRED] - D.samples(b, fmt)[BLURRED]).mean()) / (1.0 if D.max_sample(fmt) == 255 else 4.0)


# measured: (S ratio, mean absolute error before, after at sensitivity 4, after at 1, S rise at 4), errors in 8-bit gray levels
MEASURED = {"bgr24": (0.1440, 20.07, 14.88, 17.95, 1.577), "nv12": (0.1439, 22.30, 16.76, 20.03, 1.544), "p010": (0.1438, 22.36, 16.80, 20.14, 1.543)}


@pytest.mark.parametrize("fmt", sorted(MEASURED))
def test_the_blurred_frame_borrows_detail(clips, fmt):
    frames, clean = clips[fmt]
    ratio, before, after4, after1, rise = MEASURED[fmt]
    S = D.sharpness(frames, fmt)
    maps, gain, donors = D.plan(D.motion_of(N), S, R)
    print(fmt, "S", S.tolist(), "gain", gain[BLURRED].tolist(), "donors", donors.tolist())
    for nb in (BLURRED - 1, BLURRED + 1):
        assert abs(S[BLURRED] / S[nb] - ratio) < 0.01
    assert donors[BLURRED] == 4 and gain[BLURRED, R] == 0.0
    assert np.all(np.abs(gain[BLURRED, [0, 1, 3, 4]] - (1.0 - ratio)) < 0.01)
    assert np.array_equal(maps[BLURRED, R], [1, 0, 0, 0, 1, 0]) and np.allclose(maps[BLURRED, 0], [1, 0, -2.5, 0, 1, -1.0], atol=1e-12)
    assert np.allclose(maps[BLURRED, 4], [1, 0, 2.5, 0, 1, 1.0], atol=1e-12)
    assert np.isnan(maps[0, :R]).all() and np.isnan(maps[N - 1, R + 1:]).all() and not np.isnan(maps[BLURRED]).any()
    assert abs(_mae(frames, clean, fmt) - before) < 0.3
    for sens, after in ((4.0, after4), (1.0, after1)):
        val, has = D.blend(frames, maps, gain, 0, None, fmt, sens)
        out = D.assemble(frames, val, has, 0, fmt)
        err, s_out = _mae(out, clean, fmt), D.sharpness(out, fmt)
        print(fmt, "sensitivity", sens, "error", err, "S rise", s_out[BLURRED] / S[BLURRED])
        assert abs(err - after) < 0.3 and err < before - 1.5
        assert s_out[BLURRED] > S[BLURRED]
        if sens == 4.0:
            assert abs(s_out[BLURRED] / S[BLURRED] - rise) < 0.03
        # the sharp frames have donors too -- neighbours a fraction of a percent sharper -- whose gains move almost nothing
        others = [t for t in range(N) if t != BLURRED]
        assert float((out[others] != frames[others]).mean()) < 0.01
        if fmt != "bgr24":   # chroma is the source's
            assert np.array_equal(out[:, H:], frames[:, H:])
    # OpenCV's default sensitivity lends next to nothing here
    val, has = D.blend(frames, maps, gain, 0, None, fmt, 0.1)
    assert _mae(D.assemble(frames, val, has, 0, fmt), clean, fmt) > before - 0.5


def test_chunked_blend_is_one_call(clips):
    frames, _ = clips["nv12"]
    maps, gain, _ = D.plan(D.motion_of(N), D.sharpness(frames, "nv12"), R)
    whole, _ = D.blend(frames, maps, gain, 0, None, "nv12")
    for s, e in ((0, 3), (3, 5), (5, 7)):
        lo, hi = max(0, s - R), min(N, e + R)
        part, _ = D.blend(frames[lo:hi], maps[s:e], gain[s:e], s - lo, e - lo, "nv12")
        assert np.array_equal(part, whole[s:e])


def test_plan_stops_where_it_must():
    n, R3 = 9, 3
    S = np.array([10, 20, 30, 40, 5, 40, 30, 20, 10], np.int64)
    m = D.motion_of(n, (0.5, -0.25))
    m[1:, 0], m[1:, 1] = 1.01 * np.cos(0.01), 1.01 * np.sin(0.01)
    maps, gain, donors = D.plan(m, S, R3)
    assert donors.tolist() == [3, 2, 2, 0, 6, 0, 2, 2, 3]   # the sharper frames within 3; every neighbour of frame 4 is sharper
    assert gain[4, R3] == 0 and np.all(gain[4, [0, 1, 2, 4, 5, 6]] > 0) and gain[3].max() == 0.0
    assert gain[4, 2] == np.float32(1.0 - 5.0 / 40.0)
    # a chain and its inverse chain undo each other
    for t, k in ((4, 2), (2, 3), (6, -3)):
        a, b = np.vstack([maps[t, R3 + k].reshape(2, 3), [0, 0, 1]]), np.vstack([maps[t + k, R3 - k].reshape(2, 3), [0, 0, 1]])
        assert np.allclose(a @ b, np.eye(3), atol=1e-12)
    spread = np.nanmax(np.abs(maps - D.plan(m, S, R3, order="inward")[0]))
    assert 0.0 <= spread < 1e-12
    # a NaN row at 4 (the pair 3 | 4) stops every chain that would cross it, on both sides; so does a scale of 3, and so does a cut
    for bad in ("nan", "scale", "cut"):
        mm = m.copy()
        if bad == "nan":
            mm[4, 2] = np.nan
        elif bad == "scale":
            mm[4, :2] *= 3.0
        maps, gain, donors = D.plan(mm, S, R3, cuts=[4] if bad == "cut" else None)
        for t in range(n):
            for k in range(-R3, R3 + 1):
                u = t + k
                crosses = min(t, u) < 4 <= max(t, u)
                dead = not 0 <= u < n or crosses
                assert np.isnan(maps[t, R3 + k]).all() == dead and (not dead or gain[t, R3 + k] == 0), (bad, t, k)
        assert donors[4] == 3 and donors[3] == 0
    maps, gain, donors = D.plan(m, np.full(n, 7, np.int64), R3)   # equal sharpness: nobody lends
    assert donors.sum() == 0 and gain.max() == 0.0
    maps, gain, donors = D.plan(m[:1], S[:1], 2)   # one frame
    assert maps.shape == (1, 5, 6) and np.array_equal(maps[0, 2], [1, 0, 0, 0, 1, 0]) and np.isnan(maps[0, [0, 1, 3, 4]]).all() and donors[0] == 0


def test_sharpness_is_the_integer_definition():
    rs = np.random.RandomState(3)
    f = rs.randint(0, 256, (2, 5, 6, 3)).astype(np.uint8)
    want = []
    for t in range(2):
        i = [[(29 * int(p[0]) + 150 * int(p[1]) + 77 * int(p[2]) + 128) >> 8 for p in row] for row in f[t]]
        want.append(sum((i[y][x + 1] - i[y][x - 1]) ** 2 + (i[y + 1][x] - i[y - 1][x]) ** 2 for y in range(1, 4) for x in range(1, 5)))
    assert D.sharpness(f, "bgr24").tolist() == want
    assert D.sharpness(f, "bgr24", rgb=True).tolist() == D.sharpness(f[..., ::-1], "bgr24").tolist() != want
    assert D.sharpness(np.full((1, 6, 8), 77, np.uint8), "nv12").tolist() == [0]
    p = (rs.randint(0, 1024, (1, 6, 8)) << 6).astype(np.uint16)
    assert D.sharpness(p, "p010").tolist() == D.sharpness((p >> 6).astype(np.uint16), "i010").tolist()
    assert D.sharpness(np.full((1, 6, 8), 65535, np.uint16), "i010").tolist() == [0]   # clamped to 1023: flat


class _Stub:
    def __call__(self, x, is_training):
        raise AssertionError("the generator must not run")


def test_argument_checks():
    """_check_deblur, the stabiliser's constructor and plan, and the wrappers' checks that need no device."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    assert PF._check_deblur(2, 4, "x") == (2, 4.0) and PF._check_deblur(0, 0.5, "x", zero_ok=True) == (0, 0.5) and PF._check_deblur(15.0, 1, "x")[0] == 15
    for bad in (0, -1, 16, 2.5, float("nan"), None, "2", True):
        with pytest.raises(ValueError, match="radius"):
            PF._check_deblur(bad, 4.0, "x")
    for bad in (0.0, -1.0, float("nan"), float("inf"), None, "x"):
        with pytest.raises(ValueError, match="sensitivity"):
            PF._check_deblur(2, bad, "x")
    vs = S.VideoStabilizer(_Stub(), device="cpu")
    assert vs.deblur == 0 and vs.deblur_sensitivity == 4.0 and vs.deblur_sharpness is None and vs.deblur_donors is None
    frames = torch.zeros((20, 96, 128, 3), dtype=torch.uint8)
    plain = vs._plan(frames, chunk=8)
    assert plain.deblur == 0 and not plain.two_pass
    for bad in (-1, 16, 1.5):
        with pytest.raises(ValueError, match="radius"):
            S.VideoStabilizer(_Stub(), device="cpu", deblur=bad)
    with pytest.raises(ValueError, match="sensitivity"):
        S.VideoStabilizer(_Stub(), device="cpu", deblur=2, deblur_sensitivity=0.0)
    vs = S.VideoStabilizer(_Stub(), device="cpu", deblur=2, deblur_sensitivity=3.0)
    p = vs._plan(frames, chunk=8, scene_cuts=[11], in_flight=2)
    assert (p.deblur, p.deblur_sensitivity, p.two_pass, p.lattice, p.cuts) == (2, 3.0, True, False, (11,))
    assert vs._plan(torch.zeros((4, 60, 40), dtype=torch.uint16), pixel_format="p010").deblur == 2
    with pytest.raises(ValueError, match="whole clip"):
        vs._plan(frames, halo_left=2)
    with pytest.raises(ValueError, match="whole clip"):
        vs._plan(frames, halo_right=1)
    for borders in ("keep", "mosaic"):
        with pytest.raises(ValueError, match="second pass.*" + borders):
            S.VideoStabilizer(_Stub(), device="cpu", deblur=2, borders=borders)._plan(frames)
    with pytest.raises(ValueError, match="deblur=2 is for the integer pixel formats"):
        vs._plan(torch.zeros((20, 96, 128, 3)))
    vs.deblur = 16   # (set after construction: the plan reads it again)
    with pytest.raises(ValueError, match="radius"):
        vs._plan(frames)
    vs.deblur, vs.deblur_sensitivity = 2, float("nan")
    with pytest.raises(ValueError, match="sensitivity"):
        vs._plan(frames)
    assert "deblur" not in S.VideoStabilizer.run.__code__.co_varnames   # run() does not take it
    # the wrappers: float frames and host tensors are ValueErrors, before the library is touched
    maps, gain = torch.zeros((20, 5, 6), dtype=torch.float64), torch.zeros((20, 5))
    with pytest.raises(ValueError, match="integer pixel formats"):
        PF.deblur_frames(frames.float(), maps, gain)
    with pytest.raises(ValueError, match="on the device"):
        PF.deblur_frames(frames, maps, gain)
    with pytest.raises(ValueError, match="maps must be"):
        PF.deblur_frames(frames, maps[:, :4], gain)
    with pytest.raises(ValueError, match="gain must be"):
        PF.deblur_frames(frames, maps, gain.double())
    with pytest.raises(ValueError, match="range"):
        PF.deblur_frames(frames, maps, gain, 3, 2)
    with pytest.raises(ValueError, match="sensitivity"):
        PF.deblur_frames(frames, maps, gain, sensitivity=-1.0)
    with pytest.raises(ValueError, match="radius"):
        PF.deblur_frames(frames, torch.zeros((20, 33, 6), dtype=torch.float64), torch.zeros((20, 33)))
    with pytest.raises(ValueError, match="uint16"):
        PF.deblur_frames(torch.zeros((4, 60, 40), dtype=torch.uint8), maps[:4], gain[:4], pixel_format="p010")
    with pytest.raises(ValueError, match="integer pixel formats"):
        S.frame_sharpness(frames.float())
    with pytest.raises(ValueError, match="on the device"):
        S.frame_sharpness(frames)
    with pytest.raises(ValueError, match="3 x 3"):
        S.frame_sharpness(torch.zeros((1, 2, 8, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="motion must be"):
        S.deblur_plan(torch.zeros((4, 4), dtype=torch.float64), torch.zeros(4, dtype=torch.int64), 2)


def test_the_abi_declares_the_entries():
    from pwstablenet_amd import build, hipabi
    names = ("pws_frame_sharpness_u8", "pws_plane_sharpness_u8", "pws_plane_sharpness_u16", "pws_deblur_plan", "pws_deblur_u8", "pws_deblur_plane_u8",
             "pws_deblur_plane_u16")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pwstable.h")).read(), flags=re.S)
    for name in names:
        assert name in hipabi.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
        assert hipabi.SIGNATURES[name][1][-1] is hipabi.c_stream
    assert "deblur.hip" in build.SOURCES and hipabi.ABI_VERSION == 5
