"""numpy restatement of what the 4:2:2 and 4:4:4 formats of the streaming stabiliser ARE (functional.CHROMA_FORMATS), for the tests; written
from the definitions, numpy only:
  * packing.  A frame of H x W pixels is packed rows of W samples: the Y plane (H rows), then the chroma -- "nv16" / "p210": H rows of W/2
    interleaved U V pairs; "i422" / "i210": a U plane and a V plane of H x W/2; "i444" / "i410": a U plane and a V plane of H x W -- so
    (T, 2 H, W) for 4:2:2 and (T, 3 H, W) for 4:4:4.  uint8, or uint16 words with the 10-bit sample placed as the 4:2:0 format of the same
    plane order places it ("p210" as "p010": word >> 6; "i210" / "i410" as "i010": min(word, 1023)).  ``pack`` / ``unpack`` move WORDS, not
    samples: what they carry is bit for bit what the kernels read;
  * the oracle of the GPU tests, plane equivalence.  The warp, the bicubic warp and the keep pass work plane by plane and depend on nothing
    but a plane's own size, so a plane of a new-format frame must come out as the same-sized plane of a 4:2:0 frame does: ``luma_carrier``
    puts a frame's Y plane into a 4:2:0 frame of H x W, ``chroma_carrier`` its chroma into the chroma of a 4:2:0 frame of 2H x W (4:2:2, same
    plane order) or of a planar 4:2:0 frame of 2H x 2W (4:4:4); ``from_carriers`` packs the planes that come back;
  * ``yuv2bgr``: the BGR decode of the window planes -- tests/yuv_ref.py's BT.601 limited-range fixed point with the chroma of sample
    (x >> cx, y >> cy), (cx, cy) = (1, 1), (1, 0), (0, 0) for 4:2:0, 4:2:2, 4:4:4; 16-bit frames are reduced first (yuv16_ref.reduce8);
  * ``random_frames``: uniform noise over all words (16 bit: junk in P210's low bits and I210 / I410 words above 1023 included)."""
import numpy as np

#            dtype      interleaved  chroma  the 4:2:0 format of the same depth and plane order
FORMATS = {
    "nv16": (np.uint8, True, 1, "nv12"),
    "i422": (np.uint8, False, 1, "i420"),
    "p210": (np.uint16, True, 1, "p010"),
    "i210": (np.uint16, False, 1, "i010"),
    "i444": (np.uint8, False, 2, "i420"),
    "i410": (np.uint16, False, 2, "i010"),
}
FORMATS420 = {"nv12": (np.uint8, True, 0, "nv12"), "i420": (np.uint8, False, 0, "i420"),
              "p010": (np.uint16, True, 0, "p010"), "i010": (np.uint16, False, 0, "i010")}
ALL = dict(FORMATS420, **FORMATS)
SHIFTS = ((1, 1), (1, 0), (0, 0))   # (cx, cy) per chroma 0, 1, 2
NAMES8 = tuple(n for n in FORMATS if FORMATS[n][0] == np.uint8)
NAMES16 = tuple(n for n in FORMATS if FORMATS[n][0] == np.uint16)


def dtype(fmt):
    return ALL[fmt][0]


def shifts(fmt):
    return SHIFTS[ALL[fmt][2]]


def base420(fmt):
    return ALL[fmt][3]


def packed_rows(fmt, h):
    cx, cy = shifts(fmt)
    return h + ((2 * (h >> cy)) >> cx)   # two chroma planes of (h >> cy) rows of (W >> cx) samples, in rows of W


def height(fmt, rows):
    """H of a frame of ``rows`` packed rows."""
    unit = packed_rows(fmt, 2)
    assert rows % unit == 0
    return rows // unit * 2


def unpack(frames, fmt):
    """(T, packed rows, W) words -> Y (T, H, W), U and V (T, H >> cy, W >> cx), as words."""
    frames = np.asarray(frames)
    t, rows, w = frames.shape
    h = height(fmt, rows)
    cx, cy = shifts(fmt)
    c = frames[:, h:].reshape(t, -1)
    if ALL[fmt][1]:
        c = c.reshape(t, h >> cy, w >> cx, 2)
        return frames[:, :h], c[..., 0], c[..., 1]
    c = c.reshape(t, 2, h >> cy, w >> cx)
    return frames[:, :h], c[:, 0], c[:, 1]


def pack(y, u, v, fmt):
    """Planes of words -> (T, packed rows, W) of the format's dtype."""
    t, h, w = y.shape
    cx, cy = shifts(fmt)
    assert u.shape == v.shape == (t, h >> cy, w >> cx), (u.shape, (t, h >> cy, w >> cx))
    if ALL[fmt][1]:
        c = np.stack([u, v], -1).reshape(t, -1, w)
    else:
        c = np.concatenate([u.reshape(t, -1), v.reshape(t, -1)], 1).reshape(t, -1, w)
    out = np.concatenate([y, c], 1).astype(dtype(fmt))
    assert out.shape == (t, packed_rows(fmt, h), w)
    return out


def random_frames(t, h, w, fmt, seed=0):
    """Uniform noise over all words of the format's dtype."""
    rs = np.random.RandomState(seed)
    top = 256 if dtype(fmt) == np.uint8 else 65536
    return rs.randint(0, top, (t, packed_rows(fmt, h), w)).astype(dtype(fmt))


def _filler(shape, fmt, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256 if dtype(fmt) == np.uint8 else 65536, shape).astype(dtype(fmt))


def luma_carrier(frames, fmt, seed=101):
    """The 4:2:0 frames (same depth and plane order) of H x W whose Y plane is the frames' Y plane; their chroma is noise."""
    y, _, _ = unpack(frames, fmt)
    t, h, w = y.shape
    return pack(y, _filler((t, h // 2, w // 2), fmt, seed), _filler((t, h // 2, w // 2), fmt, seed + 1), base420(fmt))


def chroma_carrier(frames, fmt, seed=103):
    """The 4:2:0 frames whose chroma planes are the frames' chroma planes: 2H x W in the same plane order for 4:2:2 (chroma H x W/2), planar
    2H x 2W for 4:4:4 (chroma H x W).  Their Y plane is noise."""
    _, u, v = unpack(frames, fmt)
    t, ch, cw = u.shape
    return pack(_filler((t, 2 * ch, 2 * cw), fmt, seed), u, v, base420(fmt))


def from_carriers(luma420, chroma420, fmt):
    """The frame of ``fmt`` whose Y plane is ``luma420``'s and whose chroma planes are ``chroma420``'s."""
    y, _, _ = unpack(luma420, base420(fmt))
    _, u, v = unpack(chroma420, base420(fmt))
    return pack(y, u, v, fmt)


def from420(frames420, fmt420, fmt):
    """The frame of ``fmt`` that shows the 4:2:0 frame's picture: chroma rows repeated (4:2:2), rows and columns repeated (4:4:4)."""
    y, u, v = unpack(frames420, fmt420)
    cx, cy = shifts(fmt)
    rep = lambda c: np.repeat(np.repeat(c, 2 >> cy, 1), 2 >> cx, 2)   # noqa: E731
    return pack(y, rep(u), rep(v), fmt)


def samples10(words, fmt):
    """The 10-bit samples of 16-bit words: the interleaved formats place them as P010 does (word >> 6), the planar ones as I010 (min(word, 1023))."""
    w = np.asarray(words).astype(np.int64)
    return w >> 6 if ALL[fmt][1] else np.minimum(w, 1023)


def place10(v10, fmt):
    v = np.asarray(v10).astype(np.int64)
    return (v << 6 if ALL[fmt][1] else v).astype(np.uint16)


def samples8(words, fmt):
    """The 8-bit samples the window planes see: the bytes, or the reduction min(255, (v10 + 2) >> 2) of the 10-bit sample of each word."""
    if dtype(fmt) == np.uint8:
        return np.asarray(words).astype(np.int64)
    return np.minimum(255, (samples10(words, fmt) + 2) >> 2)


def yuv2bgr(frames, fmt):
    """(T, packed rows, W) -> (T, H, W, 3) uint8: OpenCV 4.x's 8-bit BT.601 limited-range fixed point, pixel (x, y) with the chroma of sample
    (x >> cx, y >> cy)."""
    y, u, v = (samples8(p, fmt) for p in unpack(frames, fmt))
    cx, cy = shifts(fmt)
    up = lambda c: np.repeat(np.repeat(c, 1 << cy, 1), 1 << cx, 2)   # noqa: E731
    yy = np.maximum(0, y - 16) * 1220542
    uu, vv = up(u) - 128, up(v) - 128
    r = (yy + 1673527 * vv + (1 << 19)) >> 20
    g = (yy - 852492 * vv - 409993 * uu + (1 << 19)) >> 20
    b = (yy + 2116026 * uu + (1 << 19)) >> 20
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)
