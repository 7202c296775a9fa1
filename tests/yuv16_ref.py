"""numpy restatement of the 10-bit 4:2:0 YUV path of the streaming stabiliser for the tests (P010 / I010 in, the same layout out), written
from the definitions, not from the kernels:
  * packing: a frame is (H * 3 // 2, W) uint16 in the 8-bit formats' plane order -- "p010": the Y plane, then H/2 rows of interleaved U V,
    the 10-bit sample in the HIGH bits of each word (word = v10 << 6; the low 6 bits of input words are ignored, output words have them
    zero); "i010" (yuv420p10le): Y, U and V planes, the sample in the LOW 10 bits (input words above 1023 are clamped to 1023);
  * ``reduce8``: the 8-bit reduction the generator sees, v8 = min(255, (v10 + 2) >> 2); ``window_planes`` are tests/yuv_ref.py's of the
    reduced NV12 / I420 clip;
  * ``warp_yuv``: each plane warped by the field resized (align_corners=True) to the plane's size, bilinear on the 10-bit values under the
    generator's align_corners convention, taps outside a plane read BT.601 black at 10 bits (64 in Y, 512 in U and V), truncated and
    clamped to 0..1023, stored in the format's placement; in float64, or in float32 (``dtype``) to measure what fp32 coordinates cost;
  * ``area_resize_yuv16``: INTER_AREA plane by plane on the 10-bit values (P010's UV as a 2-channel image) as cv::resize dispatches 16-bit
    unsigned images: 2 x 2 -> (a + b + c + d + 2) >> 2; integer ratios -> the block sum times float(1 / area), rounded half to even; else
    the float area tables (oracle/frameio_ref._area_tab).  PARITY UNPINNED against cv2, like oracle/frameio_ref.py: OpenCV is not installed
    here, so this follows OpenCV 4.x's documented algorithms (imgproc/resize.cpp) and could not be checked against cv2 itself.
"""
import numpy as np

import yuv_ref
from oracle import frameio_ref

PAD = {"y": 64.0, "c": 512.0}
FMT8 = {"p010": "nv12", "i010": "i420"}


def samples(words, fmt):
    """The 10-bit samples of 16-bit words in the format's placement."""
    w = np.asarray(words).astype(np.int64)
    return w >> 6 if fmt == "p010" else np.minimum(w, 1023)


def place(v10, fmt):
    v = np.asarray(v10).astype(np.int64)
    return (v << 6 if fmt == "p010" else v).astype(np.uint16)


def unpack(frames, fmt):
    """(T, H*3/2, W) words -> the 10-bit samples Y (T, H, W), U (T, H/2, W/2), V (T, H/2, W/2)."""
    return yuv_ref.unpack(samples(frames, fmt), FMT8[fmt])


def pack(y, u, v, fmt):
    """10-bit samples -> (T, H*3/2, W) uint16 words in the format's placement."""
    t, h, w = y.shape
    if fmt == "p010":
        c = np.stack([u, v], -1).reshape(t, h // 2, w)
    else:
        c = np.concatenate([u.reshape(t, -1), v.reshape(t, -1)], 1).reshape(t, h // 2, w)
    return place(np.concatenate([y, c], 1), fmt)


def reduce8(v10):
    return np.minimum(255, (np.asarray(v10).astype(np.int64) + 2) >> 2).astype(np.uint8)


def reduce(frames, fmt):
    """The NV12 / I420 clip of the reduced samples (the packing orders are the same: word for word)."""
    return reduce8(samples(frames, fmt))


def expand(frames8, fmt):
    """8-bit NV12 / I420 frames as 10-bit frames of ``fmt``: v10 = v8 << 2 (reduce(expand(f)) == f)."""
    return place(np.asarray(frames8).astype(np.int64) << 2, fmt)


def window_planes(frames, fmt, size=256):
    return yuv_ref.window_planes(reduce(frames, fmt), FMT8[fmt], size)


def _resize_field(field, ph, pw, dt):
    """UpsamplingBilinear2d(size=(ph, pw)) of (T, fh, fw, 2) (align_corners=True), every operation in ``dt``."""
    t, fh, fw, _ = field.shape
    f = field.astype(dt)
    sy = np.arange(ph).astype(dt) * dt((fh - 1) / (ph - 1) if ph > 1 else 0.0)
    sx = np.arange(pw).astype(dt) * dt((fw - 1) / (pw - 1) if pw > 1 else 0.0)
    y0, x0 = np.floor(sy).astype(int), np.floor(sx).astype(int)
    y1, x1 = np.minimum(y0 + 1, fh - 1), np.minimum(x0 + 1, fw - 1)
    ly, lx = (sy - y0.astype(dt))[None, :, None, None], (sx - x0.astype(dt))[None, None, :, None]
    one = dt(1)
    top = f[:, y0][:, :, x0] * (one - lx) + f[:, y0][:, :, x1] * lx
    bot = f[:, y1][:, :, x0] * (one - lx) + f[:, y1][:, :, x1] * lx
    return top * (one - ly) + bot * ly


def warp_plane(plane, field, align_corners, pad, dtype=np.float64):
    """plane (T, h, w[, c]) of 10-bit samples warped by field (T, fh, fw, 2) -> (the truncated 10-bit samples, the real-valued blend)."""
    dt = np.dtype(dtype).type
    p = np.asarray(plane).astype(dt)
    if p.ndim == 3:
        p = p[..., None]
    t, h, w, c = p.shape
    g = _resize_field(np.asarray(field), h, w, dt)
    one, two = dt(1), dt(2)
    if align_corners:
        ix, iy = (g[..., 0] + one) / two * dt(w - 1), (g[..., 1] + one) / two * dt(h - 1)
    else:
        ix, iy = ((g[..., 0] + one) * dt(w) - one) / two, ((g[..., 1] + one) * dt(h) - one) / two
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    wx1, wy1 = (ix - x0.astype(dt))[..., None], (iy - y0.astype(dt))[..., None]
    n = np.arange(t)[:, None, None]

    def tap(yy, xx):
        ok = ((xx >= 0) & (xx < w) & (yy >= 0) & (yy < h))[..., None]
        v = p[n, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(ok, v, dt(pad))
    out = (tap(y0, x0) * (one - wx1) * (one - wy1) + tap(y0, x0 + 1) * wx1 * (one - wy1) + tap(y0 + 1, x0) * (one - wx1) * wy1
           + tap(y0 + 1, x0 + 1) * wx1 * wy1)
    assert out.dtype == np.dtype(dtype)
    # truncation of the real-valued blend; in float64, 1e-9 absorbs its rounding (an exact integer must not truncate to its neighbour)
    eps = 1e-9 if np.dtype(dtype) == np.float64 else 0.0
    v10 = np.clip(np.floor(out.astype(np.float64) + eps), 0, 1023).astype(np.int64)
    if np.asarray(plane).ndim == 3:
        v10, out = v10[..., 0], out[..., 0]
    return v10, out.astype(np.float64)


def warp_yuv(frames, field, fmt, align_corners=False, return_float=False, dtype=np.float64):
    """The fused 10-bit warp: (T, H*3/2, W) uint16 -> the same layout (and the real-valued blend of the 10-bit values, in the 8-bit
    formats' packing order of that layout, when return_float)."""
    y, u, v = unpack(frames, fmt)
    wy, fy = warp_plane(y, field, align_corners, PAD["y"], dtype)
    if fmt == "p010":
        wc, fc = warp_plane(np.stack([u, v], -1), field, align_corners, PAD["c"], dtype)
        wu, wv, fu, fv = wc[..., 0], wc[..., 1], fc[..., 0], fc[..., 1]
    else:
        wu, fu = warp_plane(u, field, align_corners, PAD["c"], dtype)
        wv, fv = warp_plane(v, field, align_corners, PAD["c"], dtype)
    out = pack(wy, wu, wv, fmt)
    if not return_float:
        return out
    t, h, w = fy.shape
    if fmt == "p010":
        fl = np.concatenate([fy, np.stack([fu, fv], -1).reshape(t, h // 2, w)], 1)
    else:
        fl = np.concatenate([fy, np.concatenate([fu.reshape(t, -1), fv.reshape(t, -1)], 1).reshape(t, h // 2, w)], 1)
    return out, fl


def resize_area_u10(img, oh, ow):
    """cv2.resize(img (H, W, C) of 10-bit samples, (ow, oh), INTER_AREA), down-scaling, as cv::resize dispatches CV_16U -> int64 (H, W, C)."""
    img = np.asarray(img).astype(np.int64)
    h, w, c = img.shape
    if h == 2 * oh and w == 2 * ow:
        return (img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2] + 2) >> 2
    if h % oh == 0 and w % ow == 0:
        ky, kx = h // oh, w // ow
        s = img.reshape(oh, ky, ow, kx, c).sum(axis=(1, 3))
        v = (s.astype(np.float32) * np.float32(np.float32(1.0) / np.float32(kx * ky))).astype(np.float32)
        return np.clip(np.rint(v), 0, 1023).astype(np.int64)
    xt, yt = frameio_ref._area_tab(w, ow), frameio_ref._area_tab(h, oh)
    src = img.astype(np.float32)
    buf = np.zeros((h, ow, c), np.float32)   # horizontal pass, accumulated in table order in float32
    for dx, ent in enumerate(xt):
        acc = np.zeros((h, c), np.float32)
        for sx, a in ent:
            acc = (acc + src[:, sx] * a).astype(np.float32)
        buf[:, dx] = acc
    out = np.zeros((oh, ow, c), np.int64)
    for dy, ent in enumerate(yt):
        acc = None
        for sy, beta in ent:
            term = (buf[sy] * beta).astype(np.float32)
            acc = term if acc is None else (acc + term).astype(np.float32)
        out[dy] = np.clip(np.rint(acc), 0, 1023).astype(np.int64)   # rint: half to even, as cvRound
    return out


def area_resize_yuv16(frames, fmt, size):
    """INTER_AREA plane by plane on the 10-bit values: Y to (height, width), chroma to (height/2, width/2); size = (width, height)."""
    ow, oh = size
    y, u, v = unpack(frames, fmt)
    ys = np.stack([resize_area_u10(f[..., None], oh, ow)[..., 0] for f in y])
    if fmt == "p010":
        c = np.stack([resize_area_u10(np.stack([a, b], -1), oh // 2, ow // 2) for a, b in zip(u, v)])
        us, vs = c[..., 0], c[..., 1]
    else:
        us = np.stack([resize_area_u10(f[..., None], oh // 2, ow // 2)[..., 0] for f in u])
        vs = np.stack([resize_area_u10(f[..., None], oh // 2, ow // 2)[..., 0] for f in v])
    return pack(ys, us, vs, fmt)


def random_yuv16(t, h, w, fmt, seed=0, smooth=True, noise=3):
    """Plausible 10-bit 4:2:0 frames: smooth Y in [64, 940] and chroma in [64, 960] with +-``noise`` LSB of 10 bits on top (or uniform
    noise over all 16-bit words when not smooth: junk in P010's low bits and I010 words above 1023 included)."""
    rs = np.random.RandomState(seed)
    if not smooth:
        return rs.randint(0, 65536, (t, h * 3 // 2, w)).astype(np.uint16)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)

    def plane(ph, pw, lo, hi, k):
        a = rs.uniform(0, 2 * np.pi, (t, 3))
        gy, gx = yy[:ph, :pw] * (h / ph), xx[:ph, :pw] * (w / pw)
        v = sum(np.sin(gx[None] * (0.013 + 0.007 * i) + gy[None] * (0.017 - 0.004 * i) + a[:, i, None, None] + k) for i in range(3)) / 3
        return np.clip(np.round(lo + (hi - lo) * (0.5 + 0.5 * v) + rs.randint(-noise, noise + 1, (t, ph, pw))), 0, 1023).astype(np.int64)
    return pack(plane(h, w, 64, 940, 0), plane(h // 2, w // 2, 64, 960, 1), plane(h // 2, w // 2, 64, 960, 2), fmt)


def smooth_field(n, seed, scale=1.02, shift=0.01, noise=0.01, shear=0.03, size=256):
    """A stabiliser-like field (n, size, size, 2) float32: torch's F.affine_grid(theta, align_corners=False) of a small affine map plus
    white noise.  The default zooms out, so a band of taps falls outside the frame."""
    rs = np.random.RandomState(seed)
    c = ((np.arange(size, dtype=np.float32) * 2 + 1) / np.float32(size) - 1).astype(np.float32)
    xs, ys = np.meshgrid(c, c, indexing="xy")
    th = np.array([scale, shear, shift, -0.02, 2.0 - scale - 0.01, 0.02], np.float32)
    g = np.stack([th[0] * xs + th[1] * ys + th[2], th[3] * xs + th[4] * ys + th[5]], -1).astype(np.float32)
    return (g[None] + np.float32(noise) * rs.standard_normal((n, size, size, 2)).astype(np.float32)).astype(np.float32)


def inside_field(n, seed, noise=0.005, size=256):
    """smooth_field zoomed IN (both axes scaled by 0.9 about a small shift and shear, less noise): every tap stays inside every plane."""
    rs = np.random.RandomState(seed)
    c = ((np.arange(size, dtype=np.float32) * 2 + 1) / np.float32(size) - 1).astype(np.float32)
    xs, ys = np.meshgrid(c, c, indexing="xy")
    th = np.array([0.9, 0.02, 0.005, -0.02, 0.9, 0.005], np.float32)
    g = np.stack([th[0] * xs + th[1] * ys + th[2], th[3] * xs + th[4] * ys + th[5]], -1).astype(np.float32)
    return (g[None] + np.float32(noise) * rs.standard_normal((n, size, size, 2)).astype(np.float32)).astype(np.float32)


WARP_SHAPES = [(2, 720, 1280), (1, 90, 896), (2, 48, 64), (1, 38, 52)]


def warp_case(shape, fmt):
    """The inputs of the warp test of one shape, (frames, field), for the GPU test and for the CPU test that runs the restatement in
    float32 on them.  Why the wide frames get a field that stays inside: where a tap pair straddles a plane's edge the blend runs from the
    picture to black, up to 940 - 64 = 876 LSB of 10 bits per pixel of coordinate (4x an 8-bit frame's slope).  An fp32 coordinate of a
    plane W wide carries a few units of W * 2^-23 of rounding (the field's interpolation weights, the un-normalisation), about 3e-4 pixels at
    W = 1280: 0.25 LSB against black, which no fp32 evaluation keeps inside the acceptance band of 0.05 (measured on the restatement
    itself: 0.19).  Inside a smooth picture the slope is ~15 LSB per pixel and the same coordinate error moves the blend by < 0.01.  At
    W <= 128 the error against black is 876 * 3 * 128 * 2^-23 = 0.04, inside the band, so the small shapes and the border test
    (72 x 128) keep the field that zooms out and blend with black along their edges."""
    n, h, w = shape
    f = random_yuv16(n, h, w, fmt, seed=h)
    return f, (inside_field(n, seed=h) if w > 128 else smooth_field(n, seed=h))


def wide_border_case(fmt):
    """A 720p clip under the field that zooms OUT (smooth_field): the wide-plane case warp_case leaves out, taps that leave a 1280-wide Y
    plane and 640-wide chroma planes on every side.  Judged by accept_wide, not accept."""
    n, h, w = 2, 720, 1280
    return random_yuv16(n, h, w, fmt, seed=h + 1), smooth_field(n, seed=h + 1, noise=0.005)


def tap_masks(shape, field, fmt, align_corners, margin=1e-3):
    """Where the four taps of every output sample lie, from float64 coordinates, in the packing order of ``fmt`` ((T, H*3/2, W) bool each):
    ``inside`` -- the blend reads the plane only, ``outside`` -- it reads black only, both under any error of the coordinates below
    ``margin`` pixels (fp32 coordinates of a 1280-wide plane carry about 3e-4, see warp_case); neither -- the blend mixes picture and black,
    or may do so in fp32."""
    t, hh, w = shape
    h = hh * 2 // 3
    dt = np.float64

    def plane(ph, pw):
        g = _resize_field(np.asarray(field), ph, pw, dt)
        if align_corners:
            ix, iy = (g[..., 0] + 1) / 2 * (pw - 1), (g[..., 1] + 1) / 2 * (ph - 1)
        else:
            ix, iy = ((g[..., 0] + 1) * pw - 1) / 2, ((g[..., 1] + 1) * ph - 1) / 2
        ins = (ix >= margin) & (ix <= pw - 1 - margin) & (iy >= margin) & (iy <= ph - 1 - margin)
        out = (ix <= -1 - margin) | (ix >= pw + margin) | (iy <= -1 - margin) | (iy >= ph + margin)
        return ins, out
    (yi, yo), (ci, co) = plane(h, w), plane(h // 2, w // 2)
    res = []
    for ym, cm in ((yi, ci), (yo, co)):
        if fmt == "p010":
            c = np.repeat(cm, 2, 2)
        else:
            c = np.concatenate([cm.reshape(t, -1), cm.reshape(t, -1)], 1).reshape(t, h // 2, w)
        res.append(np.concatenate([ym, c], 1))
    return res


def accept_wide(got, ref_words, ref_f, fmt, inside, outside, share=6e-2, exact_black=True):
    """The acceptance function of the wide border case: at most 1 LSB of 10 bits off everywhere; where all four taps are inside the plane,
    a difference only where the float64 blend lies within 0.05 of an integer (accept's band); where all are outside, exactly black; a share
    of differing samples below accept's cap.  Where a tap pair straddles the edge of a wide plane the blend runs from the picture to black
    at up to 876 LSB per pixel, and an fp32 coordinate error of 3e-4 pixels moves it by 0.26 LSB: outside any band around the integers
    narrower than that, but never 2 LSB off.  ``exact_black`` False drops the third condition, for a plain fp32 evaluation: black times four
    weights that sum to 1 - 1 ulp truncates to one below black, which a kernel has to treat on its own to meet the definition.  Returns (the share of differing samples, the share of samples that straddle)."""
    g, r = samples(got, fmt), samples(ref_words, fmt)
    diff = np.abs(g - r)
    assert diff.max() <= 1, diff.max()
    assert bool((np.abs(ref_f - np.round(ref_f)) < 0.05)[(diff > 0) & inside].all())
    t, hh, w = g.shape
    black = np.concatenate([np.full((t, hh * 2 // 3, w), 64), np.full((t, hh // 3, w), 512)], 1)
    if exact_black:
        assert bool((np.asarray(got)[outside] == place(black, fmt)[outside]).all())
    frac = float((diff > 0).mean())
    assert frac < share, frac
    return frac, float((~inside & ~outside).mean())


def border_case(fmt):
    """The inputs of the border test: a field that moves a wide band on the right out of a 72 x 128 frame."""
    n, h, w = 2, 72, 128
    return random_yuv16(n, h, w, fmt, seed=7), smooth_field(n, seed=8, scale=1.3, shift=0.4, noise=0.0)


def accept(got, ref_words, ref_f, fmt, share=6e-2):
    """The acceptance function of the warp tests, for ``got`` against the float64 restatement (``ref_words``, ``ref_f`` of warp_yuv): at
    most 1 LSB of 10 bits off, a difference only where the float64 blend lies within 0.05 of an integer (band and cap are those of the
    8-bit test's assert_close_to_ref), a share of differing samples below ``share``.  Returns that share."""
    diff = np.abs(samples(got, fmt) - samples(ref_words, fmt))
    assert diff.max() <= 1, diff.max()
    assert bool((np.abs(ref_f - np.round(ref_f)) < 0.05)[diff > 0].all())
    frac = float((diff > 0).mean())
    assert frac < share, frac
    return frac
