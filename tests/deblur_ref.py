"""Deblurring restated on the CPU (include/pwstable.h pws_frame_sharpness_u8 / pws_deblur_plan / pws_deblur_u8 have the definitions): the
sharpness in integers, the plan and the blend in float64.  The blend takes the donor position q through the same single fp32 rounding as the
kernel, so positions -- the inside test, the tap indices, the fractions -- are shared bit for bit and only the blend's arithmetic differs."""
import numpy as np

# name -> (dtype, packed rows per 2 picture rows (None: (T, H, W, 3) pixels), how a word becomes a sample)
FORMATS = {"bgr24": (np.uint8, None, "bgr"), "nv12": (np.uint8, 3, "u8"), "i420": (np.uint8, 3, "u8"), "nv16": (np.uint8, 4, "u8"),
           "i422": (np.uint8, 4, "u8"), "i444": (np.uint8, 6, "u8"), "p010": (np.uint16, 3, "shift"), "i010": (np.uint16, 3, "clamp"),
           "p210": (np.uint16, 4, "shift"), "i210": (np.uint16, 4, "clamp"), "i410": (np.uint16, 6, "clamp")}


def frame_hw(frames, fmt):
    unit = FORMATS[fmt][1]
    return (frames.shape[1], frames.shape[2]) if unit is None else (frames.shape[1] // unit * 2, frames.shape[2])


def max_sample(fmt):
    return 255 if FORMATS[fmt][0] == np.uint8 else 1023


def samples(frames, fmt):
    """The samples that are blended, as integers: (n, h, w, 3) for bgr24, the Y plane (n, h, w) otherwise (P010: word >> 6; I010: min(word, 1023))."""
    kind = FORMATS[fmt][2]
    if kind == "bgr":
        return frames.astype(np.int64)
    h, _ = frame_hw(frames, fmt)
    y = frames[:, :h].astype(np.int64)
    return y >> 6 if kind == "shift" else np.minimum(y, 1023) if kind == "clamp" else y


def intensity(frames, fmt, rgb=False):
    v = samples(frames, fmt)
    if FORMATS[fmt][2] != "bgr":
        return v
    w0, w2 = (77, 29) if rgb else (29, 77)
    return (w0 * v[..., 0] + 150 * v[..., 1] + w2 * v[..., 2] + 128) >> 8


def sharpness(frames, fmt="bgr24", rgb=False):
    """S[t]: the sum over the interior of the squared central differences of the integer intensity, int64."""
    i = intensity(frames, fmt, rgb)
    gx = i[:, 1:-1, 2:] - i[:, 1:-1, :-2]
    gy = i[:, 2:, 1:-1] - i[:, :-2, 1:-1]
    return (gx * gx + gy * gy).reshape(len(i), -1).sum(1).astype(np.int64)


def _row_ok(m):
    if not np.isfinite(m).all():
        return False
    s = float(np.hypot(m[0], m[1]))
    return 0.5 <= s <= 2.0


def _step(m, future):
    a, b, tx, ty = (float(v) for v in m)
    if not future:
        return [a, 0.0 - b, tx, b, a, ty]
    d = a * a + b * b
    ia, ib = a / d, b / d
    return [ia, ib, 0.0 - (ia * tx + ib * ty), 0.0 - ib, ia, ib * tx - ia * ty]


def _compose(s, c):
    """s o c, row-major 2 x 3, every product and sum rounded once in the kernel's order."""
    return [s[0] * c[0] + s[1] * c[3], s[0] * c[1] + s[1] * c[4], (s[0] * c[2] + s[1] * c[5]) + s[2],
            s[3] * c[0] + s[4] * c[3], s[3] * c[1] + s[4] * c[4], (s[3] * c[2] + s[4] * c[5]) + s[5]]


def plan(motion, sharp, radius, cuts=None, order="outward"):
    """(maps (n, 2R+1, 6) float64, gain (n, 2R+1) float32, donors (n,) int32).  order="outward" is the kernel's: C_j = step_j o C_{j-1};
    "inward" multiplies the same steps from the far end, (step_j o step_{j-1}) o ...: the same map up to rounding, whose distance from the
    first is the spread that the GPU test scales its tolerance by."""
    motion, sharp = np.asarray(motion, np.float64), np.asarray(sharp, np.int64)
    n, R = len(motion), int(radius)
    K = 2 * R + 1
    maps = np.full((n, K, 6), np.nan)
    gain = np.zeros((n, K), np.float32)
    bounds = [0] + sorted(cuts or []) + [n]
    for a, b in zip(bounds[:-1], bounds[1:]):
        for t in range(a, b):
            maps[t, R] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
            for direction in (-1, 1):
                steps = []
                for j in range(1, R + 1):
                    u = t + direction * j
                    if not a <= u < b:
                        break
                    row = motion[u + 1] if direction < 0 else motion[u]
                    if not _row_ok(row):
                        break
                    steps.append(_step(row, direction > 0))
                    if order == "outward":
                        c = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
                        for s in steps:
                            c = _compose(s, c)
                    else:
                        c = steps[-1]
                        for s in steps[-2::-1]:
                            c = _compose(c, s)
                    maps[t, R + direction * j] = c
                    if sharp[u] > sharp[t]:
                        gain[t, R + direction * j] = np.float32(1.0 - float(sharp[t]) / float(sharp[u]))
    return maps, gain, (gain > 0).sum(1).astype(np.int32)


def blend(frames, maps, gain, start=0, stop=None, fmt="bgr24", sensitivity=4.0):
    """The weighted means BEFORE rounding, float64: (stop - start, h, w, 3) for bgr24, the luma (stop - start, h, w) otherwise, in sample units;
    and per frame whether it has a donor at all (a frame without one is a copy)."""
    v = samples(frames, fmt).astype(np.float64)
    n, (h, w) = len(frames), frame_hw(frames, fmt)
    stop = n if stop is None else stop
    R = (maps.shape[1] - 1) // 2
    bgr = FORMATS[fmt][2] == "bgr"
    s = float(np.float32(sensitivity)) * (1.0 if max_sample(fmt) == 255 else 4.0)
    cx, cy = 0.5 * (w - 1), 0.5 * (h - 1)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dx, dy = xx - cx, yy - cy

    def inten(a):
        return (29.0 * a[..., 0] + 150.0 * a[..., 1] + 77.0 * a[..., 2]) / 256.0 if bgr else a
    out = np.empty((stop - start,) + v.shape[1:])
    has = np.zeros(stop - start, bool)
    for i, t in enumerate(range(start, stop)):
        own = v[t]
        acc, wsum, i0 = own.copy(), np.ones((h, w)), inten(own)
        for k in list(range(-R, 0)) + list(range(1, R + 1)):
            g, u = float(gain[i, R + k]), t + k
            if not g > 0.0 or not 0 <= u < n:
                continue
            has[i] = True
            m = maps[i, R + k]
            with np.errstate(invalid="ignore"):
                qx = ((m[0] * dx + (m[1] * dy + m[2])) + cx).astype(np.float32)
                qy = ((m[3] * dx + (m[4] * dy + m[5])) + cy).astype(np.float32)
                inside = (qx >= 0) & (qx <= np.float32(w - 1)) & (qy >= 0) & (qy <= np.float32(h - 1))
            qx, qy = np.where(inside, qx, np.float32(0)), np.where(inside, qy, np.float32(0))
            x0 = np.clip(np.floor(qx), 0, w - 2).astype(np.int64)
            y0 = np.clip(np.floor(qy), 0, h - 2).astype(np.int64)
            lx, ly = qx.astype(np.float64) - x0, qy.astype(np.float64) - y0
            if bgr:
                lx, ly = lx[..., None], ly[..., None]
            d = v[u]
            top = (1.0 - lx) * d[y0, x0] + lx * d[y0, x0 + 1]
            bot = (1.0 - lx) * d[y0 + 1, x0] + lx * d[y0 + 1, x0 + 1]
            val = (1.0 - ly) * top + ly * bot
            wgt = np.where(inside, g * s / (s + np.abs(inten(val) - i0)), 0.0)
            acc += (wgt[..., None] if bgr else wgt) * val
            wsum += wgt
        out[i] = acc / (wsum[..., None] if bgr else wsum)
    return out, has


def assemble(frames, values, has, start, fmt):
    """The output frames from ``blend``'s values: rounded to the nearest integer (ties to even), clamped to the sample range and placed
    as the format places them; chroma planes, and frames without a donor, are the source's words."""
    out = frames[start:start + len(values)].copy()
    q = np.clip(np.rint(values), 0, max_sample(fmt)).astype(np.int64)
    if FORMATS[fmt][2] == "shift":
        q = q << 6
    h, _ = frame_hw(frames, fmt)
    for i in range(len(values)):
        if has[i]:
            if FORMATS[fmt][2] == "bgr":
                out[i] = q[i]
            else:
                out[i, :h] = q[i]
    return out


def texture(n, h, w, seed, velocity=(1.25, 0.5), blurred=(), taps=5, waves=16, lam=(3.0, 24.0)):
    """A translating texture, (n, h, w) float64 in [0, 1]: a sum of sinusoids moving by ``velocity`` pixels a frame (frame k shows the
    texture shifted by k * velocity, so motion row k is (1, 0, -vx, -vy)); the frames in ``blurred`` are the mean of ``taps`` horizontally
    shifted copies (a box blur, evaluated analytically).  Returns (clip, clean clip)."""
    rs = np.random.RandomState(seed)
    wl, ang, ph = rs.uniform(lam[0], lam[1], waves), rs.uniform(0, 2 * np.pi, waves), rs.uniform(0, 2 * np.pi, waves)
    amp = rs.uniform(0.5, 1.0, waves)
    kx, ky = 2 * np.pi / wl * np.cos(ang), 2 * np.pi / wl * np.sin(ang)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")

    def frame(t, shift=0.0):
        x, y = xx - t * velocity[0] + shift, yy - t * velocity[1]
        return sum(a * np.sin(p + kxx * x + kyy * y) for a, p, kxx, kyy in zip(amp, ph, kx, ky))
    norm = 2.2 * np.sqrt((amp ** 2).sum() / 2)
    clean = np.stack([0.5 + 0.5 * np.clip(frame(t) / norm, -1, 1) for t in range(n)])
    clip = clean.copy()
    for t in blurred:
        clip[t] = np.mean([0.5 + 0.5 * np.clip(frame(t, float(j - taps // 2)) / norm, -1, 1) for j in range(taps)], 0)
    return clip, clean


def motion_of(n, velocity=(1.25, 0.5)):
    m = np.tile(np.array([1.0, 0.0, -velocity[0], -velocity[1]]), (n, 1))
    m[0] = [1.0, 0.0, 0.0, 0.0]
    return m


def to_format(gray, fmt, seed=0):
    """Frames in ``fmt`` whose intensity is the (n, h, w) texture ``gray`` in [0, 1]: BGR with three tinted channels, YUV with the texture
    as luma and smooth noise as chroma."""
    dtype, unit, kind = FORMATS[fmt]
    n, h, w = gray.shape
    rs = np.random.RandomState(seed)
    if kind == "bgr":
        col = np.stack([gray * 0.9, gray, gray * 0.8], -1) * 255.0
        return np.clip(np.rint(col), 0, 255).astype(np.uint8)
    top = 255 if dtype == np.uint8 else 1023
    y = np.clip(np.rint(gray * top), 0, top).astype(np.int64)
    c = rs.randint(top // 4, 3 * top // 4, (n, h * unit // 2 - h, w))
    f = np.concatenate([y, c], 1)
    return (f << 6 if kind == "shift" else f).astype(dtype)
