"""numpy restatement of the 4:2:0 YUV path of the streaming stabiliser for the tests (semantics of csrc/frameio.hip's and
csrc/grid_sample.hip's YUV kernels, written from the definitions, not from the kernels):
  * packing: a frame is (H * 3 // 2, W) uint8, the Y plane, then NV12's H/2 rows of interleaved U V or I420's U plane and V plane;
  * ``yuv2bgr``: OpenCV 4.x's 8-bit BT.601 limited-range fixed point (COLOR_YUV2BGR_NV12 / _I420), chroma of sample (x/2, y/2), in
    integers -- unpinned against cv2, which is not available here;
  * ``warp_yuv``: each plane warped by the field resized (align_corners=True) to the plane's size, bilinear in float64 under the
    generator's align_corners convention, taps outside a plane read BT.601 black (16 in Y, 128 in U and V), truncated like astype(uint8);
  * ``area_resize_yuv``: INTER_AREA plane by plane (NV12's UV as a 2-channel image).
"""
import numpy as np

from oracle import frameio_ref

PAD = {"y": 16.0, "c": 128.0}


def unpack(frames, fmt):
    """(T, H*3/2, W) -> Y (T, H, W), U (T, H/2, W/2), V (T, H/2, W/2)."""
    frames = np.asarray(frames)
    t, ph, w = frames.shape
    h = ph // 3 * 2
    y = frames[:, :h]
    if fmt == "nv12":
        c = frames[:, h:].reshape(t, h // 2, w // 2, 2)
        return y, c[..., 0], c[..., 1]
    c = frames[:, h:].reshape(t, 2, h // 2, w // 2)
    return y, c[:, 0], c[:, 1]


def pack(y, u, v, fmt):
    t, h, w = y.shape
    if fmt == "nv12":
        c = np.stack([u, v], -1).reshape(t, h // 2, w)
    else:
        c = np.concatenate([u.reshape(t, -1), v.reshape(t, -1)], 1).reshape(t, h // 2, w)
    return np.concatenate([y, c], 1).astype(np.uint8)


def yuv2bgr(frames, fmt):
    """cv2.cvtColor(frame, COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_I420) of every frame: (T, H*3/2, W) -> (T, H, W, 3) uint8."""
    y, u, v = unpack(frames, fmt)
    up = lambda c: np.repeat(np.repeat(c.astype(np.int64), 2, 1), 2, 2)   # noqa: E731  (chroma of sample (x/2, y/2))
    yy = np.maximum(0, y.astype(np.int64) - 16) * 1220542
    uu, vv = up(u) - 128, up(v) - 128
    r = (yy + 1673527 * vv + (1 << 19)) >> 20
    g = (yy - 852492 * vv - 409993 * uu + (1 << 19)) >> 20
    b = (yy + 2116026 * uu + (1 << 19)) >> 20
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def _resize_field(field, ph, pw):
    """UpsamplingBilinear2d(size=(ph, pw)) of (T, fh, fw, 2) in float64 (align_corners=True)."""
    t, fh, fw, _ = field.shape
    f = field.astype(np.float64)
    sy = np.arange(ph) * ((fh - 1) / (ph - 1) if ph > 1 else 0.0)
    sx = np.arange(pw) * ((fw - 1) / (pw - 1) if pw > 1 else 0.0)
    y0, x0 = np.floor(sy).astype(int), np.floor(sx).astype(int)
    y1, x1 = np.minimum(y0 + 1, fh - 1), np.minimum(x0 + 1, fw - 1)
    ly, lx = (sy - y0)[None, :, None, None], (sx - x0)[None, None, :, None]
    top = f[:, y0][:, :, x0] * (1 - lx) + f[:, y0][:, :, x1] * lx
    bot = f[:, y1][:, :, x0] * (1 - lx) + f[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def warp_plane(plane, field, align_corners, pad, return_float=False):
    """plane (T, h, w[, c]) uint8 warped by field (T, fh, fw, 2) -> (T, h, w[, c]) uint8 (and the float64 blend)."""
    p = np.asarray(plane).astype(np.float64)
    if p.ndim == 3:
        p = p[..., None]
    t, h, w, c = p.shape
    g = _resize_field(np.asarray(field), h, w)
    if align_corners:
        ix, iy = (g[..., 0] + 1) / 2 * (w - 1), (g[..., 1] + 1) / 2 * (h - 1)
    else:
        ix, iy = ((g[..., 0] + 1) * w - 1) / 2, ((g[..., 1] + 1) * h - 1) / 2
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    wx1, wy1 = (ix - x0)[..., None], (iy - y0)[..., None]
    n = np.arange(t)[:, None, None]

    def tap(yy, xx):
        ok = ((xx >= 0) & (xx < w) & (yy >= 0) & (yy < h))[..., None]
        v = p[n, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(ok, v, pad)
    out = (tap(y0, x0) * (1 - wx1) * (1 - wy1) + tap(y0, x0 + 1) * wx1 * (1 - wy1) + tap(y0 + 1, x0) * (1 - wx1) * wy1
           + tap(y0 + 1, x0 + 1) * wx1 * wy1)
    # astype(uint8) of the real-valued blend; 1e-9 absorbs float64 rounding (an exact integer must not truncate to its neighbour)
    u8 = np.clip(np.floor(out + 1e-9), 0, 255).astype(np.uint8)
    if np.asarray(plane).ndim == 3:
        u8, out = u8[..., 0], out[..., 0]
    return (u8, out) if return_float else u8


def warp_yuv(frames, field, fmt, align_corners=False, return_float=False):
    """The fused YUV warp: (T, H*3/2, W) uint8 -> the same layout (and the float64 blend in that layout when return_float)."""
    y, u, v = unpack(frames, fmt)
    wy, fy = warp_plane(y, field, align_corners, PAD["y"], True)
    if fmt == "nv12":
        wc, fc = warp_plane(np.stack([u, v], -1), field, align_corners, PAD["c"], True)
        wu, wv, fu, fv = wc[..., 0], wc[..., 1], fc[..., 0], fc[..., 1]
    else:
        wu, fu = warp_plane(u, field, align_corners, PAD["c"], True)
        wv, fv = warp_plane(v, field, align_corners, PAD["c"], True)
    out = pack(wy, wu, wv, fmt)
    if not return_float:
        return out
    t, h, w = fy.shape
    if fmt == "nv12":
        fl = np.concatenate([fy, np.stack([fu, fv], -1).reshape(t, h // 2, w)], 1)
    else:
        fl = np.concatenate([fy, np.concatenate([fu.reshape(t, -1), fv.reshape(t, -1)], 1).reshape(t, h // 2, w)], 1)
    return out, fl


def area_resize_yuv(frames, fmt, size):
    """cv2.resize(plane, INTER_AREA) plane by plane: Y to (height, width), chroma to (height/2, width/2); size = (width, height)."""
    ow, oh = size
    y, u, v = unpack(frames, fmt)
    ys = np.stack([frameio_ref.resize_area_u8_hwc(f[..., None], oh, ow)[..., 0] for f in y])
    if fmt == "nv12":
        c = np.stack([frameio_ref.resize_area_u8_hwc(np.stack([a, b], -1), oh // 2, ow // 2) for a, b in zip(u, v)])
        us, vs = c[..., 0], c[..., 1]
    else:
        us = np.stack([frameio_ref.resize_area_u8_hwc(f[..., None], oh // 2, ow // 2)[..., 0] for f in u])
        vs = np.stack([frameio_ref.resize_area_u8_hwc(f[..., None], oh // 2, ow // 2)[..., 0] for f in v])
    return pack(ys, us, vs, fmt)


def window_planes(frames, fmt, size=256):
    """The generator's window planes of the BGR decode (oracle window_plane of yuv2bgr)."""
    return np.stack([frameio_ref.window_plane(f, size) for f in yuv2bgr(frames, fmt)])


def random_yuv(t, h, w, fmt, seed=0, smooth=True):
    """Plausible 4:2:0 frames: smooth Y in [16, 235] and chroma in [16, 240] (or uniform noise in 0..255 when not smooth)."""
    rs = np.random.RandomState(seed)
    if not smooth:
        return rs.randint(0, 256, (t, h * 3 // 2, w)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)

    def plane(ph, pw, lo, hi, k):
        a = rs.uniform(0, 2 * np.pi, (t, 3))
        gy, gx = yy[:ph, :pw] * (h / ph), xx[:ph, :pw] * (w / pw)
        v = sum(np.sin(gx[None] * (0.013 + 0.007 * i) + gy[None] * (0.017 - 0.004 * i) + a[:, i, None, None] + k) for i in range(3)) / 3
        return np.clip(np.round(lo + (hi - lo) * (0.5 + 0.5 * v) + rs.randint(-3, 4, (t, ph, pw))), 0, 255).astype(np.uint8)
    return pack(plane(h, w, 16, 235, 0), plane(h // 2, w // 2, 16, 240, 1), plane(h // 2, w // 2, 16, 240, 2), fmt)
