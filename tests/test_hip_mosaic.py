"""GPU tests of the "mosaic" borders kernel (csrc/border_mosaic.hip; functional.mosaic_borders_, C: pws_border_mosaic_u8 / _yuv_u8 / _yuv_u16)
against the float64 restatement tests/mosaic_ref.py.

All eleven formats x both align_corners values x both margins (bilinear 0, bicubic 1) x four fields (mosaic_ref.field_case: a shift that
ramps over the clip, the same zoomed out, a smooth random field, the identity) at keep_ref.SHAPES -- 16 x 20 (chroma width 10 = 2 mod 4),
18 x 24 (odd chroma height), 12 x 520 (rows across wave boundaries) with 8 x 8 fields -- and 720 x 1280 with a 256 x 256 field (the wave-shared
field modes) for one format per kernel kind; T = 9 frames, R = 3.  The frames under test are the project's own black-border warp of noise
sources, so neighbouring frames differ in every sample and a wrong donor shows.

Check: a sample is UNDECIDED if any frame within +-R of it has the position within delta of a coverage threshold, delta = keep_ref.FACTOR x
the plane's fp32 coordinate error (keep_ref.fp32_error; test_hip_keep.py has the derivation and the measured sizes: at most 2.6e-3 pixels).
Decided samples EQUAL the rule; an undecided one may be the sample of any frame within +-R; the undecided share is at most keep_ref.CAP
(tests/test_mosaic_ref_cpu.py holds the fields to it by the restatement alone); covered samples are byte-identical to the input;
unfilled[t] is off the reference's count by at most the number of undecided Y positions of frame t."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keep_ref as K  # noqa: E402
import mosaic_ref as M  # noqa: E402

FORMATS = list(M.FORMATS)
MODES = ["bilinear", "bicubic"]
BIG_FORMATS = ["bgr24", "nv12", "i010", "i444"]                                        # one per kernel kind
BIG_CASES = {"ramp": (False, "bilinear"), "smooth": (True, "bicubic")}                 # (align_corners, mode): two references in all


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the cached arrays are read-only)


@functools.lru_cache(maxsize=None)
def field_of(case, fs, seed):
    f = M.field_case(case, fs, seed)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def plane_ref(case, fs, seed, ph, pw, ac, m):
    """(covered, undecided) of one plane, computed once per case and shared by the formats."""
    field = field_of(case, fs, seed)
    delta = K.FACTOR * K.fp32_error(field, ph, pw, ac)
    cov, dist = K.coverage(field, ph, pw, ac, m)
    return cov, M.undecided(dist, delta, M.R)


def packed_ref(fmt, case, fs, seed, h, w, ac, m):
    """(covered, undecided) per sample in the frames' packing, and the same of the Y (BGR: pixel) plane."""
    sizes = M.plane_sizes(fmt, h, w)
    cy, uy = plane_ref(case, fs, seed, h, w, ac, m)
    cc, uc = plane_ref(case, fs, seed, *sizes[-1], ac, m)
    return M.packed(cy, cc, fmt), M.packed(uy, uc, fmt), cy, uy


@functools.lru_cache(maxsize=None)
def warped_of(fmt, case, fs, h, w, ac, mode):
    """The project's own black-border warp of noise sources: (T, ...) in the frames' packing, read-only."""
    from pwstablenet_amd import functional as PF
    rs = np.random.RandomState(h * 7 + w + len(fmt) + len(case))
    deep = M.dtype(fmt) == np.uint16
    src = rs.randint(0, 65536 if deep else 256, M.frame_shape(fmt, M.T, h, w)).astype(M.dtype(fmt))
    field_d = dev(field_of(case, fs, w))
    if fmt == "bgr24":
        out = PF.upsample_grid_sample_u8(dev(src), field_d, align_corners=ac, mode=mode)
    else:
        out = PF.upsample_grid_sample_yuv(dev(src), field_d, fmt, align_corners=ac, mode=mode)
    out = out.cpu().numpy()
    out.setflags(write=False)
    return out


def within_radius(got, warped):
    """Every sample of got[t] is the sample of some warped[t'] with |t' - t| <= R."""
    ok = np.zeros(got.shape, bool)
    n = got.shape[0]
    for k in range(-M.R, M.R + 1):
        a, b = max(0, -k), min(n, n - k)
        ok[a:b] |= got[a:b] == warped[a + k:b + k]
    return ok


def run_case(fmt, h, w, fs, case, ac, mode):
    from pwstablenet_amd import functional as PF
    m = K.margin(mode)
    cov, und, cov_y, und_y = packed_ref(fmt, case, fs, w, h, w, ac, m)
    share = float(und.mean())
    assert share <= K.CAP, share
    warped = warped_of(fmt, case, fs, h, w, ac, mode)
    buf = dev(warped)
    got, unfilled = PF.mosaic_borders_(buf, dev(field_of(case, fs, w)), M.R, pixel_format=fmt, align_corners=ac, mode=mode, return_unfilled=True)
    assert got is buf   # in place
    got, unfilled = got.cpu().numpy(), unfilled.cpu().numpy()
    want, d = M.mosaic(warped, cov, M.R)
    tag = (fmt, h, w, case, ac, mode)
    bad = (got != want) & ~und
    assert not bad.any(), tag + (int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert within_radius(got, warped).all(), tag                    # undecided samples too: never anything but a neighbour's sample
    assert np.array_equal(got[cov & ~und], warped[cov & ~und]), tag   # covered samples are untouched
    ref_unf = M.unfilled(cov_y, M.R)
    slack = und_y.reshape(M.T, -1).sum(1)
    assert unfilled.dtype == np.int32 and unfilled.shape == (M.T,)
    assert (np.abs(unfilled.astype(np.int64) - ref_unf) <= slack).all(), tag + (unfilled.tolist(), ref_unf.tolist(), slack.tolist())
    if case == "identity" and mode == "bilinear":
        assert np.array_equal(got, warped) and not unfilled.any()
    if case in ("ramp", "ramp_zoom"):
        assert not np.array_equal(got, warped)
    if case == "ramp":
        assert set(np.unique(d).tolist()) >= set(range(-M.R, M.R + 1))
    return share


@pytest.mark.parametrize("hwf", M.SHAPES, ids=lambda s: "%dx%d" % (s[0], s[1]))
@pytest.mark.parametrize("fmt", FORMATS)
def test_mosaic_small(hip, fmt, hwf):
    h, w, fs = hwf
    worst = 0.0
    for case in M.FIELDS:
        for ac in (False, True):
            for mode in MODES:
                worst = max(worst, run_case(fmt, h, w, fs, case, ac, mode))
    print("%s %dx%d: largest share of undecided samples %.5f" % (fmt, h, w, worst))


@pytest.mark.parametrize("case", list(BIG_CASES))
@pytest.mark.parametrize("fmt", BIG_FORMATS)
def test_mosaic_720p(hip, fmt, case):
    h, w, fs = M.BIG
    ac, mode = BIG_CASES[case]
    print("%s 720p %s ac=%s %s: share of undecided samples %.6f" % (fmt, case, ac, mode, run_case(fmt, h, w, fs, case, ac, mode)))


@pytest.mark.parametrize("fmt", FORMATS)
def test_start_and_stop(hip, fmt):
    """Filling [3, 6) changes no other frame and gives the whole-range call's bytes for those three; [0, 4) then [4, 9) equals one call."""
    from pwstablenet_amd import functional as PF
    h, w, fs = M.SHAPES[1]
    for case, ac, mode in (("ramp", False, "bilinear"), ("ramp_zoom", True, "bicubic")):
        warped = warped_of(fmt, case, fs, h, w, ac, mode)
        field = dev(field_of(case, fs, w))
        kw = dict(pixel_format=fmt, align_corners=ac, mode=mode, return_unfilled=True)
        whole, unf = PF.mosaic_borders_(dev(warped), field, M.R, **kw)
        whole, unf = whole.cpu().numpy(), unf.cpu().numpy()
        assert not np.array_equal(whole[3:6], warped[3:6])
        part, unf_part = PF.mosaic_borders_(dev(warped), field, M.R, 3, 6, **kw)
        part = part.cpu().numpy()
        assert np.array_equal(part[:3], warped[:3]) and np.array_equal(part[6:], warped[6:])
        assert np.array_equal(part[3:6], whole[3:6]) and np.array_equal(unf_part.cpu().numpy(), unf[3:6])
        buf = dev(warped)
        _, ua = PF.mosaic_borders_(buf, field, M.R, 0, 4, **kw)
        assert np.array_equal(buf[4:].cpu().numpy(), warped[4:])
        _, ub = PF.mosaic_borders_(buf, field, M.R, 4, None, **kw)
        assert np.array_equal(buf.cpu().numpy(), whole)
        assert np.array_equal(torch.cat([ua, ub]).cpu().numpy(), unf)
        _, u0 = PF.mosaic_borders_(buf, field, M.R, 5, 5, **kw)   # an empty range: nothing changes
        assert u0.numel() == 0 and np.array_equal(buf.cpu().numpy(), whole)


def test_unfilled_is_written_not_accumulated(hip):
    A = hip
    h, w, fs = M.SHAPES[0]
    warped = warped_of("nv12", "ramp_zoom", fs, h, w, False, "bilinear")
    field, buf = dev(field_of("ramp_zoom", fs, w)), dev(warped)
    unf = torch.full((M.T,), 12345, dtype=torch.int32, device="cuda")
    rc = A.lib().pws_border_mosaic_yuv_u8(A.ptr(buf), A.ptr(field), A.ptr(unf), M.T, 0, M.T, M.R, h, w, fs, fs, 0, 0, 0, 0, A.current_stream())
    assert rc == 0
    cov_y, und_y = plane_ref("ramp_zoom", fs, w, h, w, False, 0)
    got = unf.cpu().numpy()
    assert got.max() < 12345 and got.sum() > 0 and (np.abs(got - M.unfilled(cov_y, M.R)) <= und_y.reshape(M.T, -1).sum(1)).all()


def test_argument_checks(hip):
    from pwstablenet_amd import functional as PF
    A = hip
    lib, st, p = A.lib(), A.current_stream(), A.ptr
    EINVAL = -22
    field = torch.zeros((4, 4, 4, 2), device="cuda")
    u8 = torch.zeros(4 * 16 * 16 * 3, dtype=torch.uint8, device="cuda")
    u16 = torch.zeros(4 * 16 * 16 * 3, dtype=torch.uint16, device="cuda")
    unf = torch.zeros(4, dtype=torch.int32, device="cuda")
    # (frames, field, unfilled, n, start, stop, radius, h, w, fh, fw, [layout, chroma,] align_corners, bicubic, stream)
    bgr = lambda n, a, b, r, h=8, w=8, fr=u8: lib.pws_border_mosaic_u8(p(fr), p(field), p(unf), n, a, b, r, h, w, 4, 4, 0, 0, st)   # noqa: E731
    assert bgr(4, 0, 4, 1) == 0 and bgr(4, 0, 4, 15) == 0 and bgr(4, 2, 2, 3) == 0
    assert bgr(4, 0, 4, 0) == EINVAL and b"radius" in lib.pws_last_error()
    assert bgr(4, 0, 4, 16) == EINVAL and bgr(4, 0, 4, -1) == EINVAL
    assert bgr(4, -1, 4, 3) == EINVAL and b"start" in lib.pws_last_error()
    assert bgr(4, 3, 2, 3) == EINVAL and bgr(4, 0, 5, 3) == EINVAL
    assert bgr(4, 0, 4, 3, w=6) == EINVAL and bgr(4, 0, 4, 3, h=0) == EINVAL and bgr(4, 0, 4, 3, fr=u8[1:]) == EINVAL
    assert lib.pws_border_mosaic_u8(p(u8), p(field), None, 4, 0, 4, 3, 8, 8, 4, 4, 0, 0, st) == EINVAL   # NULL unfilled
    for fn, buf in ((lib.pws_border_mosaic_yuv_u8, u8), (lib.pws_border_mosaic_yuv_u16, u16)):
        yuv = lambda n, a, b, r, h=8, w=8, lay=0, chroma=0, bic=0: fn(p(buf), p(field), p(unf), n, a, b, r, h, w, 4, 4, lay, chroma, 0, bic, st)   # noqa: E731,B023
        assert yuv(4, 0, 4, 3) == 0 and yuv(4, 0, 4, 3, chroma=1) == 0 and yuv(4, 0, 4, 3, lay=1, chroma=2) == 0 and yuv(4, 1, 3, 15, bic=1) == 0
        assert yuv(4, 0, 4, 0) == EINVAL and yuv(4, 0, 4, 16) == EINVAL and yuv(4, 2, 1, 3) == EINVAL and yuv(4, 0, 5, 3) == EINVAL
        assert yuv(4, 0, 4, 3, h=7) == EINVAL and yuv(4, 0, 4, 3, w=6) == EINVAL and yuv(4, 0, 4, 3, lay=2) == EINVAL
        assert yuv(4, 0, 4, 3, chroma=3) == EINVAL and yuv(4, 0, 4, 3, lay=0, chroma=2) == EINVAL   # interleaved 4:4:4 is not offered
        assert yuv(4, 0, 4, 3, w=4) == 0 and yuv(4, 0, 4, 3, w=4, bic=1) == EINVAL                   # w >= 8 with the bicubic margin
    torch.cuda.synchronize()
    frames = torch.zeros((4, 8, 8, 3), dtype=torch.uint8, device="cuda")
    for r in (0, 16, -3):
        with pytest.raises(ValueError, match="radius"):
            PF.mosaic_borders_(frames, field, r)
    for a, b in ((-1, 4), (3, 2), (0, 5)):
        with pytest.raises(ValueError, match="range"):
            PF.mosaic_borders_(frames, field, 3, a, b)
    with pytest.raises(ValueError, match="integer pixel formats"):   # float frames
        PF.mosaic_borders_(torch.zeros((4, 3, 8, 8), device="cuda"), field, 3)
    with pytest.raises(ValueError, match="contiguous"):
        PF.mosaic_borders_(torch.zeros((4, 8, 16, 3), dtype=torch.uint8, device="cuda")[:, :, ::2], field, 3)
    with pytest.raises(ValueError, match="contiguous"):
        PF.mosaic_borders_(torch.zeros((8, 12, 8), dtype=torch.uint8, device="cuda")[::2], field, 3, pixel_format="nv12")
    with pytest.raises(ValueError, match="field"):
        PF.mosaic_borders_(frames, field[:3], 3)
    with pytest.raises(ValueError, match="field"):
        PF.mosaic_borders_(frames, torch.zeros((4, 4, 4, 3), device="cuda"), 3)
    with pytest.raises(ValueError):     # an unknown format or mode
        PF.mosaic_borders_(frames, field, 3, pixel_format="yuv444")
    with pytest.raises(ValueError):
        PF.mosaic_borders_(frames, field, 3, mode="lanczos")
    with pytest.raises(ValueError):     # dtype / format mismatch
        PF.mosaic_borders_(torch.zeros((4, 12, 8), dtype=torch.uint8, device="cuda"), field, 3, pixel_format="p010")
    with pytest.raises(RuntimeError):   # PWS_EINVAL through functional: w % 4
        PF.mosaic_borders_(torch.zeros((4, 8, 6, 3), dtype=torch.uint8, device="cuda"), field, 3)
    out, unfilled = PF.mosaic_borders_(frames[:0], field[:0], 3, return_unfilled=True)   # an empty clip
    assert out.shape[0] == 0 and unfilled.numel() == 0
    assert PF.mosaic_borders_(frames, field, 3) is frames
    assert PF.BORDERS == ("black", "keep", "mosaic") and PF.lookup_format("i444").mosaic_entry == "pws_border_mosaic_yuv_u8"
    assert PF.lookup_format("bgr24").mosaic_entry == "pws_border_mosaic_u8" and PF.lookup_format("p010").mosaic_entry == "pws_border_mosaic_yuv_u16"
