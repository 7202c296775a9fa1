"""GPU tests of deblurring's three steps (csrc/deblur.hip) against tests/deblur_ref.py: ``frame_sharpness`` in exact integers, ``deblur_plan``
with its stopping rules, and ``functional.deblur_frames`` -- every sample within 0.5 + delta of the float64 restatement, which shares the
donor positions bit for bit, and the cases that must come out exact.  Shapes are the smallest at which the kernels can go wrong: bgr24 at
50 x 38 (a width that is no multiple of 4, eight workgroups a frame), the packed formats at 52 x 40 (three workgroups), 7 frames at R = 2,
5 frames at R = 15 (the window clipped at both ends) and R = 1."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deblur_ref as D  # noqa: E402

FORMATS = ("bgr24", "nv12", "i420", "p010", "i010", "nv16", "i444", "i410")


def _hw(fmt):
    return (38, 50) if fmt == "bgr24" else (40, 52)


def _noise(fmt, n, h, w, seed, wild=False):
    """Noise frames in ``fmt``; wild: 16-bit words use all 16 bits (P010 low bits set, I010 words above 1023)."""
    dtype, unit, kind = D.FORMATS[fmt]
    rs = np.random.RandomState(seed)
    if kind == "bgr":
        return rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    rows = h * unit // 2
    if dtype == np.uint8:
        return rs.randint(0, 256, (n, rows, w)).astype(np.uint8)
    if wild:
        return rs.randint(0, 65536, (n, rows, w)).astype(np.uint16)
    v = rs.randint(0, 1024, (n, rows, w))
    return (v << 6 if kind == "shift" else v).astype(np.uint16)


def _dev(a):
    return torch.from_numpy(a).cuda()


@pytest.mark.parametrize("fmt", FORMATS + ("i422", "p210", "i210"))
def test_sharpness_is_exact(hip, fmt):
    from pwstablenet_amd import stream as S
    h, w = _hw(fmt)
    f = _noise(fmt, 3, h, w, 5, wild=True)
    f[1] = f[1, 0, 0]   # a flat frame
    got = S.frame_sharpness(_dev(f), fmt)
    want = D.sharpness(f, fmt)
    assert got.dtype == torch.int64 and got.is_cuda and got.cpu().numpy().tolist() == want.tolist() and want[1] == 0 and want[0] > 0
    sh, sw = (3, 3) if fmt == "bgr24" else (4, 4)   # the smallest frames with an interior
    small = _noise(fmt, 2, sh, sw, 6)
    assert S.frame_sharpness(_dev(small), fmt).cpu().numpy().tolist() == D.sharpness(small, fmt).tolist()
    if fmt == "bgr24":
        rgb = S.frame_sharpness(_dev(f), fmt, frames_are_rgb=True).cpu().numpy()
        assert rgb.tolist() == D.sharpness(f, fmt, rgb=True).tolist() and rgb[0] != want[0]
        big = _noise(fmt, 1, 300, 270, 7)   # more rows than row workgroups, more columns than threads
        assert S.frame_sharpness(_dev(big), fmt).cpu().numpy().tolist() == D.sharpness(big, fmt).tolist()
        out = torch.full((3,), -1, dtype=torch.int64, device="cuda")   # the entry zeroes its output itself
        assert S.frame_sharpness(_dev(f), fmt, out=out) is out and out.cpu().numpy().tolist() == want.tolist()


def _motion(n, seed):
    rs = np.random.RandomState(seed)
    ang, sc = rs.uniform(-0.02, 0.02, n), rs.uniform(0.98, 1.02, n)
    m = np.stack([sc * np.cos(ang), sc * np.sin(ang), rs.uniform(-3, 3, n), rs.uniform(-2, 2, n)], 1)
    m[0] = [1, 0, 0, 0]
    return m


PLAN_CASES = {"plain-7-2": (7, 2, None, None), "plain-5-15": (5, 15, None, None), "plain-9-1": (9, 1, None, None), "nan-row": (9, 3, "nan", None),
              "scale-3": (9, 3, "scale", None), "cut": (9, 3, None, [4]), "equal": (7, 2, "equal", None), "one-frame": (1, 2, None, None),
              "two-cuts-600": (600, 4, None, [100, 101])}


@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_plan_against_the_restatement(hip, case):
    from pwstablenet_amd import stream as S
    n, R, bad, cuts = PLAN_CASES[case]
    m = _motion(n, 3)
    sharp = np.random.RandomState(4).randint(1000, 2000, n).astype(np.int64) * 1000003
    if bad == "nan":
        m[4, 3] = np.nan
    elif bad == "scale":
        m[4, :2] *= 3.0
    elif bad == "equal":
        sharp[:] = 12345
    maps, gain, donors = S.deblur_plan(_dev(m), _dev(sharp), R, scene_cuts=cuts)
    assert (maps.dtype, gain.dtype, donors.dtype) == (torch.float64, torch.float32, torch.int32)
    maps, gain, donors = maps.cpu().numpy(), gain.cpu().numpy(), donors.cpu().numpy()
    rmaps, rgain, rdonors = D.plan(m, sharp, R, cuts)
    assert maps.shape == (n, 2 * R + 1, 6) and np.array_equal(gain, rgain) and np.array_equal(donors, rdonors)
    assert np.array_equal(np.isnan(maps), np.isnan(rmaps)) and np.array_equal(np.isnan(maps).any(2), np.isnan(maps).all(2))
    ok = ~np.isnan(rmaps)
    spread = float(np.abs(rmaps[ok] - D.plan(m, sharp, R, cuts, order="inward")[0][ok]).max())
    err = float(np.abs(maps[ok] - rmaps[ok]).max())
    print(case, "maps error %.3g, spread of the composition orders %.3g" % (err, spread))
    assert err <= max(16.0 * spread, 1e-12)
    assert np.array_equal(maps[:, R], np.tile([1.0, 0, 0, 0, 1.0, 0], (n, 1))) and not gain[:, R].any()
    if bad == "equal" or n == 1:
        assert donors.sum() == 0
    elif bad or cuts == [4]:
        assert np.isnan(maps[3, R + 1]).all() and np.isnan(maps[4, R - 1]).all() and gain[3, R + 1:].max() == 0.0


def _random_gain(n, R, seed):
    rs = np.random.RandomState(seed)
    g = rs.uniform(0.0, 1.0, (n, 2 * R + 1)).astype(np.float32)
    g[rs.uniform(size=g.shape) < 0.3] = 0.0
    g[:, R] = 0.0
    return g


BLEND_CASES = [(fmt, 7, 2) for fmt in FORMATS] + [("bgr24", 5, 15), ("nv12", 5, 15), ("p010", 5, 15), ("bgr24", 7, 1), ("i010", 7, 1)]
_CACHE = {}


def _blend_case(fmt, n, R):
    """Frames, maps, gains and the float64 restatement of one case, computed once."""
    key = (fmt, n, R)
    if key not in _CACHE:
        h, w = _hw(fmt)
        clip, _ = D.texture(n, h, w, 21, blurred=(n // 2,))
        frames = D.to_format(clip, fmt, 2)
        maps, _, _ = D.plan(_motion(n, 8), np.arange(n, dtype=np.int64) + 1, R)   # a little rotation and scale: fractional positions, some outside
        gain = _random_gain(n, R, 9)
        _CACHE[key] = (frames, maps, gain) + D.blend(frames, maps, gain, 0, None, fmt, 4.0)
    return _CACHE[key]


@pytest.mark.parametrize("fmt,n,R", BLEND_CASES, ids=["%s-%d-%d" % c for c in BLEND_CASES])
def test_blend_against_float64(hip, fmt, n, R):
    """Every sample: |out - ref| <= 0.5 + delta, delta = 64 (2R+1) 2^-24 x the largest sample value -- the rounding to an integer, plus 64 fp32
    ulps of the largest value per term of the weighted mean, the room its fp32 arithmetic gets."""
    from pwstablenet_amd import functional as PF
    frames, maps, gain, ref, has = _blend_case(fmt, n, R)
    h, w = _hw(fmt)
    out = PF.deblur_frames(_dev(frames), _dev(maps), _dev(gain), pixel_format=fmt)
    assert out.shape == frames.shape and out.dtype == _dev(frames).dtype
    out = out.cpu().numpy()
    assert has.sum() >= n // 2 and float(np.abs(ref - D.samples(frames, fmt)).max()) > 2.0   # a real blend: it moves samples by more than the bound
    delta = 64.0 * (2 * R + 1) * 2.0 ** -24 * D.max_sample(fmt)
    err = np.abs(D.samples(out, fmt) - ref)
    print("%s n %d R %d: largest |out - ref| %.6f of %.6f allowed" % (fmt, n, R, float(err.max()), 0.5 + delta))
    assert float(err.max()) <= 0.5 + delta
    if fmt != "bgr24":
        assert np.array_equal(out[:, h:], frames[:, h:])   # chroma: the source's
        if D.FORMATS[fmt][2] == "shift":
            assert not (out[:, :h] & 63).any()


@pytest.mark.parametrize("fmt", FORMATS)
def test_exact_cases(hip, fmt):
    from pwstablenet_amd import functional as PF
    h, w = _hw(fmt)
    n, R = 5, 2
    K = 2 * R + 1
    f = _noise(fmt, n, h, w, 11)
    fd = _dev(f)
    ident = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (n, K, 1))
    gain = _random_gain(n, R, 12)
    gain[gain == 0] = 0.25   # every neighbour lends
    gain[:, R] = 0.0
    # (a) all gains zero: the input, wild words included (a frame without donors is a copy)
    wild = _noise(fmt, n, h, w, 13, wild=True)
    assert torch.equal(PF.deblur_frames(_dev(wild), _dev(ident), torch.zeros((n, K), device="cuda"), pixel_format=fmt), _dev(wild))
    # (b) identical frames under the identity
    same = np.repeat(f[:1], n, 0)
    assert torch.equal(PF.deblur_frames(_dev(same), _dev(ident), _dev(gain), pixel_format=fmt), _dev(same))
    # (c) donors that are the frame shifted by whole pixels: frame t shows the big picture from (8 + 3 t, 8 + 2 t)
    dtype, unit, kind = D.FORMATS[fmt]
    big = _noise(fmt if kind == "bgr" else "i444" if dtype == np.uint8 else "i410", 1, h + 16, w + 24 + (-(w + 24)) % 4, 14)[0]
    shifted = f.copy()
    maps = ident.copy()
    for t in range(n):
        if kind == "bgr":
            shifted[t] = big[8 + 2 * t:8 + 2 * t + h, 8 + 3 * t:8 + 3 * t + w]
        else:
            y = big[8 + 2 * t:8 + 2 * t + h, 8 + 3 * t:8 + 3 * t + w]
            shifted[t, :h] = (y << 6) if kind == "shift" else y
        for k in range(-R, R + 1):
            maps[t, R + k, 2], maps[t, R + k, 5] = -3.0 * k, -2.0 * k   # position p of frame t is position p - k (3, 2) of frame t+k
    got = PF.deblur_frames(_dev(shifted), _dev(maps), _dev(gain), pixel_format=fmt)
    assert torch.equal(got, _dev(shifted))
    # (d) every q outside the frame
    far = ident.copy()
    far[:, :, 2], far[:, :, 5] = 1000.0, -1000.0
    far[:, R] = ident[:, R]
    assert torch.equal(PF.deblur_frames(fd, _dev(far), _dev(gain), pixel_format=fmt), fd)
    # (e) [start, stop) calls over the padded clip give the bytes of one call; `out` is filled in place
    maps, _, _ = D.plan(_motion(n, 15), np.arange(n, dtype=np.int64) + 1, R)
    whole = PF.deblur_frames(fd, _dev(maps), _dev(gain), pixel_format=fmt)
    assert not torch.equal(whole, fd)
    for s, e in ((0, 2), (2, 3), (3, 5)):
        lo, hi = max(0, s - R), min(n, e + R)
        out = torch.empty_like(fd[s:e])
        part = PF.deblur_frames(fd[lo:hi], _dev(maps[s:e]), _dev(gain[s:e]), s - lo, e - lo, pixel_format=fmt, out=out)
        assert part is out and torch.equal(part, whole[s:e])
    assert PF.deblur_frames(fd, _dev(maps[:0]), _dev(gain[:0]), 2, 2, pixel_format=fmt).shape[0] == 0
