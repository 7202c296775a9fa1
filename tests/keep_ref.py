"""numpy float64 restatement of the "keep" borders (functional.keep_borders_, VideoStabilizer(borders="keep")) for the tests, written from
the definition, not from the kernel.  For one plane of h x w samples and frame t:
  * coordinates: bicubic_ref.coordinates -- the field resized to the plane's own size (align_corners=True), un-normalised with the generator's
    convention; the position the fused warps sample at;
  * coverage: ``m <= ix <= w-1-m`` and ``m <= iy <= h-1-m``, m = 0 for the bilinear warp (4 taps inside), 1 for the bicubic one (16 taps);
    a NaN coordinate is not covered.  ``coverage`` also returns every pixel's distance from the nearest of the four thresholds;
  * one step: ``out[t] = covered ? warped[t] : out[t-1]`` (``step``); out[a-1] of a scene [a, b) is the scene's first SOURCE frame read as the
    warp would write it (``initial_frame``: swap_rb for BGR, P010 words masked to v10 << 6, I010 words clamped to 1023);
  * planes: Y; NV12's / P010's interleaved UV as one 2-channel plane of h/2 x w/2 positions; I420's / I010's U and V; BGR as one 3-channel
    plane -- ``packed_coverage`` lays the per-plane masks out in the frames' own packing.
``coordinates32`` evaluates the kernels' fp32 operation sequence (csrc/warp_common.h: mul_rounded, field_lerp as fma chains, one fma for
the un-normalisation) in numpy float32, an fma being the float64 product and sum rounded once more to float32; the GPU test derives its
``delta`` from its distance to the float64 coordinates."""
import numpy as np

import bicubic_ref

YUV8, YUV16 = ("nv12", "i420"), ("p010", "i010")
INTERLEAVED = ("nv12", "p010")


def margin(mode):
    return {"bilinear": 0, "bicubic": 1}[mode]


def coordinates(field, h, w, align_corners):
    """(ix, iy), each (T, h, w) float64."""
    return bicubic_ref.coordinates(field, h, w, align_corners)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def coordinates32(field, h, w, align_corners):
    """(ix, iy), each (T, h, w) float32: the kernels' own operations, in their order."""
    f = np.asarray(field, np.float32)
    t, fh, fw, _ = f.shape
    f32 = np.float32
    ry = f32(fh - 1) / f32(h - 1) if h > 1 else f32(0)
    rx = f32(fw - 1) / f32(w - 1) if w > 1 else f32(0)
    sy = (ry * np.arange(h, dtype=np.float32)).astype(np.float32)
    sx = (rx * np.arange(w, dtype=np.float32)).astype(np.float32)
    y0, x0 = sy.astype(np.int64), np.floor(sx).astype(np.int64)
    y1, x1 = y0 + (y0 < fh - 1), x0 + (x0 < fw - 1)
    ly, lx = (sy - y0.astype(np.float32)).astype(np.float32), (sx - x0.astype(np.float32)).astype(np.float32)
    hy, hx = (f32(1) - ly).astype(np.float32), (f32(1) - lx).astype(np.float32)
    ly, hy = ly[None, :, None, None], hy[None, :, None, None]
    lx, hx = lx[None, None, :, None], hx[None, None, :, None]
    a, b, c, d = f[:, y0][:, :, x0], f[:, y0][:, :, x1], f[:, y1][:, :, x0], f[:, y1][:, :, x1]
    shape = a.shape
    lxb, hxb, lyb, hyb = (np.broadcast_to(v, shape) for v in (lx, hx, ly, hy))
    top = _fma(lxb, b, (hxb * a).astype(np.float32))
    bot = _fma(lxb, d, (hxb * c).astype(np.float32))
    g = _fma(lyb, bot, (hyb * top).astype(np.float32))
    kx = f32(0.5) * f32(w - 1) if align_corners else f32(0.5) * f32(w)
    ky = f32(0.5) * f32(h - 1) if align_corners else f32(0.5) * f32(h)
    kx1, ky1 = f32(0.5) * f32(w - 1), f32(0.5) * f32(h - 1)
    full = np.ones(shape[:3], np.float32)
    return _fma(g[..., 0], kx * full, kx1 * full), _fma(g[..., 1], ky * full, ky1 * full)


def fp32_error(field, h, w, align_corners):
    """The largest distance of a finite fp32 coordinate of this plane from its float64 value, in pixels."""
    x64, y64 = coordinates(field, h, w, align_corners)
    x32, y32 = coordinates32(field, h, w, align_corners)
    return float(max(np.abs(x32 - x64).max(), np.abs(y32 - y64).max()))


def covered(ix, iy, h, w, m):
    with np.errstate(invalid="ignore"):
        return (ix >= m) & (ix <= w - 1 - m) & (iy >= m) & (iy <= h - 1 - m)   # (every comparison with NaN is False)


def coverage(field, h, w, align_corners, m):
    """(covered (T, h, w) bool, distance (T, h, w) float64 of ix / iy from the nearest of the thresholds m, w-1-m, m, h-1-m)."""
    ix, iy = coordinates(field, h, w, align_corners)
    dist = np.minimum(np.minimum(np.abs(ix - m), np.abs(ix - (w - 1 - m))), np.minimum(np.abs(iy - m), np.abs(iy - (h - 1 - m))))
    return covered(ix, iy, h, w, m), dist


def plane_sizes(fmt, h, w):
    return [(h, w)] if fmt == "bgr24" else [(h, w), (h // 2, w // 2)]


def _pack(y, c, fmt):
    """per-plane values (T, h, w) and (T, h/2, w/2) in the packing of ``fmt``: (T, h*3/2, w)."""
    t = y.shape[0]
    if fmt in INTERLEAVED:
        cc = np.repeat(c, 2, 2)
    else:
        cc = np.concatenate([c.reshape(t, -1), c.reshape(t, -1)], 1).reshape(t, y.shape[1] // 2, y.shape[2])
    return np.concatenate([y, cc], 1)


def packed_coverage(field, fmt, h, w, align_corners, m):
    """coverage of every SAMPLE of the frames, in their own layout: (T, h, w, 3) for "bgr24", (T, h*3/2, w) for the 4:2:0 formats."""
    cy, dy = coverage(field, h, w, align_corners, m)
    if fmt == "bgr24":
        return np.repeat(cy[..., None], 3, -1), np.repeat(dy[..., None], 3, -1)
    cc, dc = coverage(field, h // 2, w // 2, align_corners, m)
    return _pack(cy, cc, fmt), _pack(dy, dc, fmt)


def initial_frame(frame, fmt, is_source, swap_rb=False):
    """The frame the recurrence starts from: an earlier output frame as it is, or a source frame as the warp would write it."""
    f = np.asarray(frame)
    if not is_source:
        return f.copy()
    if fmt == "bgr24":
        return np.ascontiguousarray(f[..., ::-1]) if swap_rb else f.copy()
    if fmt == "p010":
        return (f & np.uint16(0xffc0)).astype(np.uint16)
    if fmt == "i010":
        return np.minimum(f, np.uint16(1023)).astype(np.uint16)
    return f.copy()


def step(prev, warped_t, covered_t):
    """out[t] from out[t-1]: arrays of one frame's layout."""
    return np.where(covered_t, warped_t, prev)


def keep_clip(warped, field, sources, fmt, align_corners, m, scene_cuts=(), swap_rb=False):
    """The whole recurrence over a clip: warped / sources (T, ...) in the frames' layout, scenes split at ``scene_cuts``."""
    cov, _ = packed_coverage(field, fmt, *_hw(warped, fmt), align_corners, m)
    out = np.empty_like(warped)
    for t in range(warped.shape[0]):
        prev = initial_frame(sources[t], fmt, True, swap_rb) if t == 0 or t in scene_cuts else out[t - 1]
        out[t] = step(prev, warped[t], cov[t])
    return out


def _hw(frames, fmt):
    return (frames.shape[1], frames.shape[2]) if fmt == "bgr24" else (frames.shape[1] * 2 // 3, frames.shape[2])


# ---------------------------------------------------------------- the inputs of tests/test_hip_keep.py (the CPU test checks their condition)
T = 4
SHAPES = [(16, 20, 8), (18, 24, 8), (12, 520, 8)]   # (H, W, field size): chroma width 2 mod 4; odd chroma height; rows across wave boundaries
BIG = (720, 1280, 256)                              # the wave-shared field modes
FIELDS = ["identity", "shift", "outside", "smooth"]
FACTOR = 4.0   # delta = FACTOR x the largest |fp32 - float64| coordinate: op-order freedom in the field's interpolation
CAP = 0.01     # share of a case's pixels that may lie within delta of a threshold


def field_case(case, size, seed):
    """(T, size, size, 2) float32, as test_hip_bicubic.field_case builds them: the identity's base grid (every pixel covered); a shift (about 16 % of the width to
    the right, 11 % of the height up: a wedge on two sides, its edge away from every pixel centre); everything far outside; yuv16_ref's
    smooth random field (zooms out, white noise: a ragged rim on all four sides)."""
    import yuv16_ref
    if case == "identity":   # (the 8 x 8 field is drawn in by 0.77: it also serves chroma planes of 6 and 8 rows, no larger than itself)
        return bicubic_ref.affine_field(T, size, size, scale=1.0 if size > 8 else 0.77)
    if case == "shift":
        f = bicubic_ref.affine_field(T, size, size, shift=(0.3171, -0.2237))
        f[1::2] = bicubic_ref.affine_field(T, size, size, shift=(-0.1913, 0.1321))[1::2]   # odd frames: the opposite two sides
        return f
    if case == "outside":
        return bicubic_ref.affine_field(T, size, size, shift=(3e4, -3e4))
    return yuv16_ref.smooth_field(T, seed, size=size) if size > 8 else yuv16_ref.smooth_field(T, seed, scale=1.3, size=size)   # (8 x 8 spans +-0.875 only)
