"""numpy float64 restatement of the edge modes (functional.edge_borders_, VideoStabilizer(edge="clamp" | "mirror")) for the tests, written from
the definition, not from the kernel.

Planes, coordinates and coverage are keep's (tests/keep_ref.py, which takes them from bicubic_ref.coordinates): a plane is Y, the interleaved
UV as one 2-channel plane, planar U and V, or BGR as one 3-channel plane, each of its own size for 4:2:0, 4:2:2 and 4:4:4; a position is
covered iff ``m <= ix <= W-1-m`` and ``m <= iy <= H-1-m``, m = 0 for bilinear and 1 for bicubic; NaN is not covered.

An UNCOVERED position with finite (ix, iy) becomes
    Q( sum_i sum_j wy_i wx_j v(fold(y0 + i, H), fold(x0 + j, W)) ),   x0 = floor(ix), y0 = floor(iy),
taps 0, 1 with weights (1 - t, t) for bilinear, taps -1 .. 2 with bicubic_ref.weights (A = -0.75) for bicubic;
    fold(i, n) = min(max(i, 0), n - 1)                                         for "clamp",
    fold(i, n) = k < n ? k : 2 (n - 1) - k with k = i mod 2 (n - 1); 0 if n == 1   for "mirror" (OpenCV's BORDER_REFLECT_101);
v is the SOURCE frame's sample as the warp reads it (swap_rb; P010 word >> 6; I010 min(word, 1023)); Q is bicubic_ref.quantize (clamp to the
sample range, truncate), written as the warp writes it (P010 v10 << 6).  Covered positions and positions with a non-finite coordinate keep
the warp's words.  ``sample_plane`` evaluates the sum as the first tap plus the weighted differences from it -- the same number in exact
arithmetic -- so that taps which all hold one value give that value exactly in any precision, which is part of the definition.

Planes travel channel-last, (T, h, w, C) with C = 1, 2 or 3 (``planes`` / ``unplanes``: chroma_ref's packing, which also covers the 4:2:0
formats); ``values`` / ``place`` are the read and write rules.  ``case_reference`` is the whole reference of one test case and ``check_plane``
the acceptance per sample; tests/test_hip_edge.py applies them to the device's result, tests/test_edge_ref_cpu.py to the restatement itself
evaluated in float32 on keep_ref.coordinates32."""
import functools

import numpy as np

import bicubic_ref
import chroma_ref
import keep_ref as K
import yuv16_ref
import yuv_ref

EDGES = ("clamp", "mirror")
MODES = ("bilinear", "bicubic")
FORMATS = ["bgr24", "bgr24-swap", "nv12", "i420", "p010", "i010", "nv16", "i422", "i444", "p210", "i210", "i410"]
BAND, SHARE = 0.05, 6e-2   # yuv16_ref.accept's: a difference only where the float64 blend is this close to an integer; the share that may differ


def fold(i, n, edge):
    """Tap index i of an axis of n samples, folded into [0, n)."""
    i = np.asarray(i, np.int64)
    if edge == "clamp":
        return np.clip(i, 0, n - 1)
    if edge != "mirror":
        raise ValueError(edge)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    k = np.mod(i, period)   # (numpy's mod: the divisor's sign, 0 <= k < period)
    return np.where(k < n, k, period - k)


def taps(mode):
    return {"bilinear": (0, 1), "bicubic": (-1, 0, 1, 2)}[mode]


def axis_weights(t, mode):
    return [1 - t, t] if mode == "bilinear" else bicubic_ref.weights(t)


def sample_plane(plane, ix, iy, edge, mode, where=None, dtype=np.float64):
    """plane (T, h, w[, C]) of sample VALUES, sampled at (ix, iy) (each (T, ho, wo): the warps' are the plane's own size) with the plane
    continued by ``edge``: the real-valued blend at the positions ``where`` (bool (T, ho, wo); default all) as (N, C) ``dtype``, in
    np.nonzero(where) order.  Not clamped."""
    p = np.asarray(plane)
    if p.ndim == 3:
        p = p[..., None]
    t, h, w, c = p.shape
    if where is None:
        where = np.ones(np.shape(ix), bool)
    n = np.nonzero(where)[0]
    x, y = np.asarray(ix)[where].astype(dtype), np.asarray(iy)[where].astype(dtype)
    x0, y0 = np.floor(x), np.floor(y)
    wx, wy = axis_weights(x - x0, mode), axis_weights(y - y0, mode)
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    tp = taps(mode)
    xs, ys = [fold(x0 + d, w, edge) for d in tp], [fold(y0 + d, h, edge) for d in tp]
    base = p[n, ys[0], xs[0]].astype(dtype)
    acc = np.zeros(base.shape, dtype)
    for i in range(len(tp)):
        for j in range(len(tp)):
            acc += (wy[i] * wx[j]).astype(dtype)[:, None] * (p[n, ys[i], xs[j]].astype(dtype) - base)
    return base + acc


# ---------------------------------------------------------------- formats: planes, read and write rules
def split(fmt_name):
    """("bgr24", True) for "bgr24-swap": the format and swap_rb."""
    return fmt_name.split("-")[0], fmt_name.endswith("swap")


def dtype(fmt):
    return np.uint8 if fmt == "bgr24" else chroma_ref.dtype(fmt)


def vmax(fmt):
    return 255 if dtype(fmt) == np.uint8 else 1023


def frame_shape(fmt, t, h, w):
    return (t, h, w, 3) if fmt == "bgr24" else (t, chroma_ref.packed_rows(fmt, h), w)


def planes(frames, fmt):
    """The planes of frames in their own layout, as words, channel-last: [(T, h, w, 3)] for BGR; [Y, UV] or [Y, U, V] for packed YUV."""
    frames = np.asarray(frames)
    if fmt == "bgr24":
        return [frames]
    y, u, v = chroma_ref.unpack(frames, fmt)
    if chroma_ref.ALL[fmt][1]:
        return [y[..., None], np.stack([u, v], -1)]
    return [y[..., None], u[..., None], v[..., None]]


def unplanes(pl, fmt):
    if fmt == "bgr24":
        return np.asarray(pl[0]).astype(np.uint8)
    if chroma_ref.ALL[fmt][1]:
        return chroma_ref.pack(pl[0][..., 0], pl[1][..., 0], pl[1][..., 1], fmt)
    return chroma_ref.pack(pl[0][..., 0], pl[1][..., 0], pl[2][..., 0], fmt)


def values(words, fmt):
    """The samples as the warp reads them."""
    return np.asarray(words).astype(np.int64) if dtype(fmt) == np.uint8 else chroma_ref.samples10(words, fmt)


def place(vals, fmt):
    """The words as the warp writes them."""
    return np.asarray(vals).astype(np.uint8) if dtype(fmt) == np.uint8 else chroma_ref.place10(vals, fmt)


def source_planes(src, fmt, swap_rb=False):
    """The source's planes as sample values, BGR with swap_rb applied: what ``v`` of the definition reads."""
    out = [values(p, fmt) for p in planes(src, fmt)]
    return [out[0][..., ::-1]] if fmt == "bgr24" and swap_rb else out


def fill(warped, src, field, fmt, edge, mode, align_corners, swap_rb=False):
    """The whole rule on frames in their own layout, from float64 coordinates: (T, ...) words."""
    m = K.margin(mode)
    out = []
    for wp, vals in zip(planes(warped, fmt), source_planes(src, fmt, swap_rb)):
        ph, pw = vals.shape[1:3]
        ix, iy = K.coordinates(field, ph, pw, align_corners)
        sel = ~K.covered(ix, iy, ph, pw, m) & np.isfinite(ix) & np.isfinite(iy)
        res = np.array(wp)
        res[sel] = place(bicubic_ref.quantize(sample_plane(vals, ix, iy, edge, mode, sel), vmax(fmt)), fmt)
        out.append(res)
    return unplanes(out, fmt)


# ---------------------------------------------------------------- the inputs of tests/test_hip_edge.py (the CPU test checks their condition)
T, SHAPES, BIG, FIELDS, FACTOR, CAP = K.T, K.SHAPES, K.BIG, K.FIELDS, K.FACTOR, K.CAP
# the 720 x 1280 case of each format: (field, align_corners, mode, edge) -- two combinations, so the float64 coordinates are computed twice per plane size
BIG_A, BIG_B = ("smooth", False, "bilinear", "mirror"), ("shift", True, "bicubic", "clamp")
BIG_CASE = {"bgr24": BIG_A, "bgr24-swap": BIG_B, "nv12": BIG_B, "i420": BIG_A, "p010": BIG_A, "i010": BIG_B,
            "nv16": BIG_A, "i422": BIG_B, "i444": BIG_B, "p210": BIG_B, "i210": BIG_A, "i410": BIG_A}


def small_cases():
    """(field, align_corners, mode, edge) of the small shapes: everything with everything, the plane geometry changing slowest."""
    return [(case, ac, mode, edge) for case in FIELDS for ac in (False, True) for mode in MODES for edge in EDGES]


def compares(case, edge):
    """False for "mirror" under the "outside" field: at ~3e4 plane widths the fp32 floor no longer decides the tap, so no value is compared."""
    return not (case == "outside" and edge == "mirror")


@functools.lru_cache(maxsize=None)
def field_of(case, fs, seed):
    f = K.field_case(case, fs, seed)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def source_of(fmt, h, w):
    """The smooth SOURCE frames of a case, (T, ...) in the frames' layout, read-only: the frames the warp tests use -- yuv_ref.random_yuv,
    yuv16_ref.random_yuv16 (+-3 LSB of noise on smooth planes); BGR is three such Y planes; a 4:2:2 / 4:4:4 frame takes its Y plane from such
    a frame of h x w and its chroma planes from the chroma of one of 2h x w / 2h x 2w, whose chroma planes have its chroma's size
    (chroma_ref.from_carriers).  Smooth, because equality of copies is not what is checked: the kernel's fp32 coordinates differ from the
    float64 ones by up to 6.4e-4 pixels, which on noise -- up to 1023 LSB per pixel -- moves a blend by far more than the band (measured with
    chroma_ref.random_frames as "p210" sources at 720 x 1280, smooth field, bilinear mirror: the restatement itself in float32 leaves 190 of
    157 335 uncovered samples differing outside the band; the 8 x 8-field shapes stay inside it)."""
    if fmt == "bgr24":
        f = np.stack([yuv_ref.unpack(yuv_ref.random_yuv(T, h, w, "i420", seed=h + 11 * k), "i420")[0] for k in range(3)], -1)
    elif fmt in chroma_ref.FORMATS420:
        f = (yuv_ref.random_yuv if dtype(fmt) == np.uint8 else yuv16_ref.random_yuv16)(T, h, w, fmt, seed=h)
    else:
        base = chroma_ref.base420(fmt)
        draw = yuv_ref.random_yuv if dtype(fmt) == np.uint8 else yuv16_ref.random_yuv16
        cx, cy = chroma_ref.shifts(fmt)
        f = chroma_ref.from_carriers(draw(T, h, w, base, seed=h), draw(T, h << (1 - cy), w << (1 - cx), base, seed=h + 1), fmt)
    f = np.ascontiguousarray(f)
    f.setflags(write=False)
    return f


def warped_of(fmt_name, h, w):
    """Random words, so that an untouched sample is recognisable (any words: junk in P010's low bits, I010 words above 1023)."""
    fmt, _ = split(fmt_name)
    rs = np.random.RandomState(h * 7 + w + len(fmt_name))
    return rs.randint(0, 256 if dtype(fmt) == np.uint8 else 65536, frame_shape(fmt, T, h, w)).astype(dtype(fmt))


def fp32_error(ix, iy, x32, y32):
    """keep_ref.fp32_error over the finite coordinates (a field with NaN or inf nodes has others)."""
    ok = np.isfinite(ix) & np.isfinite(iy) & np.isfinite(x32) & np.isfinite(y32)
    if not ok.any():
        return 0.0
    return float(max(np.abs(x32[ok] - ix[ok]).max(), np.abs(y32[ok] - iy[ok]).max()))


@functools.lru_cache(maxsize=8)
def _geometry(field_key, ph, pw, ac):
    field = _FIELDS[field_key]
    ix, iy = K.coordinates(field, ph, pw, ac)
    x32, y32 = K.coordinates32(field, ph, pw, ac)
    return ix, iy, x32, y32, FACTOR * fp32_error(ix, iy, x32, y32)


_FIELDS = {}


def geometry(field, key, ph, pw, ac):
    """(ix, iy float64, ix, iy float32 by the kernels' operations, delta) of one plane size under ``field``; ``key`` names the field."""
    _FIELDS[key] = field
    return _geometry(key, ph, pw, ac)


def plane_reference(vals, field, key, ac, mode, edge, fmt, float32=False):
    """The reference of one plane: vals (T, h, w, C) source sample values.  A dict of
    cov, decided, finite (T, h, w) bool -- covered; further than delta from every threshold; both coordinates finite (float64 AND fp32: a
        node the two disagree on -- 0 x inf -- belongs to neither class and is left out of ``need`` and of ``stay``);
    need (T, h, w) -- positions the rule may have filled: finite and not (covered and decided); f (N, C) the float64 blend and q (N, C) its
        quantised value there; stay (T, h, w) -- positions that must hold the warp's words: covered and decided, or not finite in both;
    f32 (N, C), only with ``float32``: the restatement in float32 on the fp32 coordinates."""
    ph, pw = vals.shape[1:3]
    m = K.margin(mode)
    ix, iy, x32, y32, delta = geometry(field, key, ph, pw, ac)
    fin64, fin32 = np.isfinite(ix) & np.isfinite(iy), np.isfinite(x32) & np.isfinite(y32)
    cov = K.covered(ix, iy, ph, pw, m)
    with np.errstate(invalid="ignore"):
        dist = np.minimum(np.minimum(np.abs(ix - m), np.abs(ix - (pw - 1 - m))), np.minimum(np.abs(iy - m), np.abs(iy - (ph - 1 - m))))
        decided = dist > delta
    finite = fin64 & fin32
    need = finite & ~(cov & decided)
    f = sample_plane(vals, ix, iy, edge, mode, need)
    ref = dict(cov=cov, decided=decided, finite=finite, need=need, stay=(finite & cov & decided) | (~fin64 & ~fin32), f=f,
               q=bicubic_ref.quantize(f, vmax(fmt)), delta=delta)
    if float32:
        ref["f32"] = sample_plane(vals, x32, y32, edge, mode, need, np.float32)
    return ref


def case_reference(fmt_name, h, w, fs, case, ac, mode, edge, float32=False):
    """(source frames, field, [plane_reference per plane]) of one case of the GPU test."""
    fmt, swap = split(fmt_name)
    src, field = source_of(fmt, h, w), field_of(case, fs, w)
    refs = [plane_reference(v, field, (case, fs, w), ac, mode, edge, fmt, float32) for v in source_planes(src, fmt, swap)]
    return src, field, refs


def check_plane(got, warped, ref, fmt, tag=(), compare=True):
    """The acceptance of one plane: got, warped (T, h, w, C) words.  Positions that must stay hold the warp's words.  An uncovered, decided
    sample is at most 1 LSB from the float64 value, differs only where the float64 blend lies within BAND of an integer, and is written as
    the warp writes (P010: low bits zero; at most 1023).  An undecided sample is either that or the warp's word.  ``compare`` False (mirror
    at ~3e4 plane widths, where fp32's floor no longer decides the tap): only the stay rule and the write rule.
    Returns (differing, uncovered decided) sample counts."""
    got, warped = np.asarray(got), np.asarray(warped)
    stay = ref["stay"]
    bad = (got != warped)[stay]
    assert not bad.any(), tag + ("a covered or non-finite sample changed", int(bad.sum()))
    need = ref["need"]
    g, wv = got[need], warped[need]
    unc, dec = ~ref["cov"][need][:, None], ref["decided"][need][:, None]
    gv = values(g, fmt)
    written = place(gv, fmt) == g
    if not compare:
        ok = np.where(unc & dec, written, written | (g == wv))
        assert ok.all(), tag + ("write rule", int((~ok).sum()))
        return 0, int((unc & dec).sum()) * g.shape[1]
    diff = np.abs(gv - ref["q"])
    f = ref["f"]
    filled = written & (diff <= 1) & ((diff == 0) | (np.abs(f - np.round(f)) < BAND))
    ok = np.where(unc & dec, filled, filled | (g == wv))
    assert ok.all(), tag + ("samples off the rule", int((~ok).sum()), float(diff[~ok].max()), np.argwhere(~ok)[:4].tolist())
    sel = np.broadcast_to(unc & dec, diff.shape)
    return int((diff[sel] > 0).sum()), int(sel.sum())


def check_case(got, warped, refs, fmt_name, tag=(), compare=True):
    """check_plane over the planes of frames in their own layout; at most SHARE of the case's uncovered decided samples may differ.
    Returns (that share, the share of undecided positions)."""
    fmt, _ = split(fmt_name)
    nd = nu = 0
    und = tot = 0
    for gp, wp, ref in zip(planes(got, fmt), planes(warped, fmt), refs):
        und, tot = und + int((~ref["decided"]).sum()), tot + ref["decided"].size
        assert (~ref["decided"]).mean() <= CAP, tag + ("undecided", float((~ref["decided"]).mean()))
        a, b = check_plane(gp, wp, ref, fmt, tag, compare)
        nd, nu = nd + a, nu + b
    share = nd / nu if nu else 0.0
    assert share <= SHARE, tag + ("share of differing samples", share)
    return share, und / tot


def restated32(warped, refs, fmt_name):
    """The frames the restatement gives in float32 on the fp32 coordinates (refs from ``case_reference(float32=True)``): fills ``need``."""
    fmt, _ = split(fmt_name)
    out = []
    for wp, ref in zip(planes(warped, fmt), refs):
        res = np.array(wp)
        blend = np.nan_to_num(ref["f32"].astype(np.float64), nan=0.0)
        res[ref["need"]] = place(bicubic_ref.quantize(blend, vmax(fmt)), fmt)
        out.append(res)
    return unplanes(out, fmt)


def nonfinite_field(fs=8):
    """keep_ref's shift field with NaN and inf nodes inside: positions that interpolate them have no finite coordinate."""
    f = np.array(field_of("shift", fs, 0))
    f[0, 2, 3, 0], f[1, 4, 4, 1], f[2, 3, 2, 0], f[3, 5, 5, 1] = np.nan, np.inf, -np.inf, np.nan
    return f
