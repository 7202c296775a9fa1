"""numpy float64 restatement of the bicubic fused warp (functional.upsample_grid_sample*(mode="bicubic")) for the tests, written from the
definition, not from the kernels.  For a plane of h x w samples with pad value ``pad``:
  * coordinates: the field resized to the plane's own size with align_corners=True (yuv16_ref._resize_field), un-normalised with the
    generator's convention -- ix = ((gx + 1) w - 1) / 2 for align_corners False, (gx + 1) / 2 (w - 1) for True; iy alike;
  * weights: x0 = floor(ix), t = ix - x0, A = -0.75, c1(s) = ((A+2)s - (A+3))s^2 + 1, c2(s) = ((As - 5A)s + 8A)s - 4A; columns x0-1 .. x0+2 weigh
    [c2(t+1), c1(t), c1(1-t), c2(2-t)], rows y0-1 .. y0+2 alike (Keys' cubic convolution, torch's grid_sample(mode="bicubic"));
  * blend: out = sum_i sum_j wy_i wx_j v(y0-1+i, x0-1+j), a tap outside the plane reading ``pad`` -- evaluated as pad + sum w (v - pad) over the
    taps inside, so a pixel whose 16 taps all lie outside is ``pad`` exactly;
  * integer outputs: clamped to [0, 255] or [0, 1023], then truncated (``quantize``); float output is not clamped.
``pad`` is 0 for float and BGR frames, 16 / 128 for 8-bit Y / chroma, 64 / 512 for 10-bit.  P010 / I010 sample placement, ignored low bits
and chroma siting are tests/yuv16_ref.py's; packing is tests/yuv_ref.py's."""
import numpy as np

import yuv16_ref
import yuv_ref

A = -0.75


def c1(s):
    return ((A + 2) * s - (A + 3)) * s * s + 1


def c2(s):
    return ((A * s - 5 * A) * s + 8 * A) * s - 4 * A


def weights(t):
    """The four weights of taps floor - 1 .. floor + 2 at fraction t."""
    return [c2(t + 1), c1(t), c1(1 - t), c2(2 - t)]


def coordinates(field, h, w, align_corners):
    """(ix, iy), each (T, h, w) float64: where every sample of an h x w plane reads."""
    g = yuv16_ref._resize_field(np.asarray(field), h, w, np.float64)
    if align_corners:
        return (g[..., 0] + 1) / 2 * (w - 1), (g[..., 1] + 1) / 2 * (h - 1)
    return ((g[..., 0] + 1) * w - 1) / 2, ((g[..., 1] + 1) * h - 1) / 2


def all_outside(field, h, w, align_corners):
    """(T, h, w) bool: the 16 taps all lie outside the plane."""
    ix, iy = coordinates(field, h, w, align_corners)
    x0, y0 = np.floor(ix), np.floor(iy)
    return (x0 + 2 < 0) | (x0 - 1 > w - 1) | (y0 + 2 < 0) | (y0 - 1 > h - 1)


def warp_plane(plane, field, align_corners, pad):
    """plane (T, h, w[, c]) warped by field (T, fh, fw, 2) -> the real-valued blend (T, h, w[, c]) float64, not clamped."""
    p = np.asarray(plane).astype(np.float64)
    squeeze = p.ndim == 3
    if squeeze:
        p = p[..., None]
    t, h, w, c = p.shape
    ix, iy = coordinates(field, h, w, align_corners)
    x0, y0 = np.floor(ix), np.floor(iy)
    wx, wy = weights(ix - x0), weights(iy - y0)
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    n = np.arange(t)[:, None, None]
    acc = np.zeros((t, h, w, c))
    for i in range(4):
        for j in range(4):
            yy, xx = y0 - 1 + i, x0 - 1 + j
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            v = p[n, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] - pad
            acc += np.where(ok, wy[i] * wx[j], 0.0)[..., None] * v
    out = acc + pad
    return out[..., 0] if squeeze else out


def quantize(blend, vmax):
    """The integer rule: clamp to [0, vmax], then truncate (1e-9 absorbs float64 rounding: an exact integer keeps its value)."""
    return np.floor(np.clip(blend, 0, vmax) + 1e-9).astype(np.int64)


def warp_bgr(frames, field, align_corners=False, swap_rb=False):
    """(T, H, W, 3) uint8 -> (the uint8 result, the float64 blend); swap_rb: output channel c samples input channel 2 - c."""
    f = np.asarray(frames)
    fl = warp_plane(f[..., ::-1] if swap_rb else f, field, align_corners, 0.0)
    return quantize(fl, 255).astype(np.uint8), fl


def warp_nchw(x, field, align_corners=False):
    """(T, C, H, W) float -> (T, C, H, W) float64, not clamped."""
    return warp_plane(np.asarray(x).transpose(0, 2, 3, 1), field, align_corners, 0.0).transpose(0, 3, 1, 2)


def _warp_packed(y, u, v, field, interleaved, align_corners, pad, vmax):
    """The planes' quantised samples and blends, chroma interleaved (NV12 / P010) warped as one 2-channel plane."""
    fy = warp_plane(y, field, align_corners, pad["y"])
    if interleaved:
        fc = warp_plane(np.stack([u, v], -1), field, align_corners, pad["c"])
        fu, fv = fc[..., 0], fc[..., 1]
    else:
        fu, fv = warp_plane(u, field, align_corners, pad["c"]), warp_plane(v, field, align_corners, pad["c"])
    return [quantize(f, vmax) for f in (fy, fu, fv)], (fy, fu, fv)


def _pack_float(fy, fu, fv, interleaved):
    t, h, w = fy.shape
    if interleaved:
        c = np.stack([fu, fv], -1).reshape(t, h // 2, w)
    else:
        c = np.concatenate([fu.reshape(t, -1), fv.reshape(t, -1)], 1).reshape(t, h // 2, w)
    return np.concatenate([fy, c], 1)


def warp_yuv(frames, field, fmt, align_corners=False):
    """(T, H*3/2, W) uint8 "nv12" / "i420" -> (the same layout uint8, the float64 blend in that layout)."""
    q, fl = _warp_packed(*yuv_ref.unpack(frames, fmt), field, fmt == "nv12", align_corners, yuv_ref.PAD, 255)
    return yuv_ref.pack(*q, fmt), _pack_float(*fl, fmt == "nv12")


def warp_yuv16(frames, field, fmt, align_corners=False):
    """(T, H*3/2, W) uint16 "p010" / "i010" -> (the same layout uint16, the float64 blend of the 10-bit values in that layout)."""
    q, fl = _warp_packed(*yuv16_ref.unpack(frames, fmt), field, fmt == "p010", align_corners, yuv16_ref.PAD, 1023)
    return yuv16_ref.pack(*q, fmt), _pack_float(*fl, fmt == "p010")


def outside_yuv(field, h, w, interleaved, align_corners):
    """all_outside of every sample of a packed 4:2:0 frame (T, h*3/2, w), in the packing order of NV12 (interleaved) or I420."""
    oy, oc = all_outside(field, h, w, align_corners), all_outside(field, h // 2, w // 2, align_corners)
    t = oy.shape[0]
    c = np.repeat(oc, 2, 2) if interleaved else np.concatenate([oc.reshape(t, -1), oc.reshape(t, -1)], 1).reshape(t, h // 2, w)
    return np.concatenate([oy, c], 1)


def affine_field(n, fh, fw, scale=1.0, shift=(0.0, 0.0), noise=0.0, seed=0):
    """A field (n, fh, fw, 2) float32: the identity's base grid (align_corners=False: (2 i + 1) / size - 1) scaled about the centre, shifted,
    plus white noise.  At the plane's own power-of-two size, scale 1 and no shift the align_corners=False coordinates are exact integers."""
    xs = ((np.arange(fw, dtype=np.float32) * 2 + 1) / np.float32(fw) - 1).astype(np.float32)
    ys = ((np.arange(fh, dtype=np.float32) * 2 + 1) / np.float32(fh) - 1).astype(np.float32)
    gx, gy = np.meshgrid(xs, ys, indexing="xy")
    g = np.stack([np.float32(scale) * gx + np.float32(shift[0]), np.float32(scale) * gy + np.float32(shift[1])], -1).astype(np.float32)
    g = np.broadcast_to(g, (n, fh, fw, 2)).copy()
    if noise:
        g += np.float32(noise) * np.random.RandomState(seed).standard_normal(g.shape).astype(np.float32)
    return g.astype(np.float32)
