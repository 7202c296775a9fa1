"""numpy float64 restatement of the "mosaic" borders (functional.mosaic_borders_, VideoStabilizer(borders="mosaic")) for the tests, written
from the definition, not from the kernel.

Planes, coordinates and coverage are keep's (tests/keep_ref.py, which takes them from bicubic_ref.coordinates): a plane is Y, the interleaved
UV as one 2-channel plane, planar U and V, or BGR as one 3-channel plane, each of its own size for 4:2:0, 4:2:2 and 4:4:4; a position is
covered iff ``m <= ix <= W-1-m`` and ``m <= iy <= H-1-m``, m = 0 for bilinear and 1 for bicubic; NaN is not covered.  Nothing is added to them.

With ``W[t]`` the frames as the black-border warp wrote them, ``C[t]`` their coverage, frames 0 .. n-1 one scene and R the radius
(1 <= R <= 15), position p of frame t:
  * ``C[t][p]``: ``out[t][p] = W[t][p]``, untouched;
  * otherwise k = 1, 2, .., R in this order: ``t-k >= 0`` and ``C[t-k][p]``: ``out[t][p] = W[t-k][p]`` (the past wins a tie); else
    ``t+k < n`` and ``C[t+k][p]``: ``out[t][p] = W[t+k][p]``;
  * no donor within R: ``out[t][p] = W[t][p]``, and the position counts as unfilled.
``donors`` returns the distance (0 covered, -k / +k, NONE unfilled), ``mosaic`` the frames, ``fill_range_`` the in-place pass over
``[start, stop)`` that reads its donors from the buffer as it is (filled frames included), ``unfilled`` the per-frame count of positions
without a donor.  ``packed`` lays per-plane values out sample by sample in the packing of each of the eleven formats."""
import numpy as np

import bicubic_ref
import keep_ref

NONE = 99   # the donor distance of a position without a donor

#           dtype     interleaved  (cx, cy): a chroma plane is (H >> cy) x (W >> cx)
FORMATS = {
    "bgr24": (np.uint8, None, None),
    "nv12": (np.uint8, True, (1, 1)), "i420": (np.uint8, False, (1, 1)), "p010": (np.uint16, True, (1, 1)), "i010": (np.uint16, False, (1, 1)),
    "nv16": (np.uint8, True, (1, 0)), "i422": (np.uint8, False, (1, 0)), "p210": (np.uint16, True, (1, 0)), "i210": (np.uint16, False, (1, 0)),
    "i444": (np.uint8, False, (0, 0)), "i410": (np.uint16, False, (0, 0)),
}


def dtype(fmt):
    return FORMATS[fmt][0]


def plane_sizes(fmt, h, w):
    """The sizes of the planes whose coverage a frame has: [Y or BGR] and, for packed YUV, the chroma planes' common size."""
    if fmt == "bgr24":
        return [(h, w)]
    cx, cy = FORMATS[fmt][2]
    return [(h, w), (h >> cy, w >> cx)]


def frame_shape(fmt, t, h, w):
    if fmt == "bgr24":
        return (t, h, w, 3)
    (ch, cw) = plane_sizes(fmt, h, w)[1]
    return (t, h + 2 * ch * cw // w, w)


def packed(y, c, fmt):
    """Per-position values y (T, h, w) and c (T, ch, cw) as per-SAMPLE values in the frames' own packing (``frame_shape``): a BGR pixel's three
    samples share y; an interleaved UV pair shares c; planar U and V each carry c."""
    t = y.shape[0]
    if fmt == "bgr24":
        return np.repeat(y[..., None], 3, -1)
    if FORMATS[fmt][1]:
        cc = np.repeat(c[..., None], 2, -1).reshape(t, -1)
    else:
        cc = np.concatenate([c.reshape(t, -1), c.reshape(t, -1)], 1)
    return np.concatenate([y, cc.reshape(t, -1, y.shape[2])], 1)


def donors(cov, radius):
    """(T, ...) int: 0 where covered, -k / +k where frame t-k / t+k is the donor, NONE where no frame within ``radius`` covers the position."""
    cov = np.asarray(cov, bool)
    n = cov.shape[0]
    d = np.where(cov, 0, NONE)
    for t in range(n):
        for k in range(1, radius + 1):
            open_ = d[t] == NONE
            if t - k >= 0:
                d[t][open_ & cov[t - k]] = -k
                open_ = d[t] == NONE
            if t + k < n:
                d[t][open_ & cov[t + k]] = k
    return d


def take(frames, d, t):
    """Frame t after the rule, its donors read from ``frames``."""
    out = frames[t].copy()
    for k in np.unique(d[t]):
        if k != 0 and k != NONE:
            sel = d[t] == k
            out[sel] = frames[t + k][sel]
    return out


def mosaic(warped, cov, radius):
    """(the frames after the rule, the donor distances): the whole scene at once, every donor read from ``warped``."""
    d = donors(cov, radius)
    return np.stack([take(warped, d, t) for t in range(warped.shape[0])]), d


def fill_range_(frames, cov, radius, start, stop):
    """The in-place pass over frames [start, stop): donors are read from ``frames`` as it is, earlier fills included."""
    d = donors(cov, radius)
    for t in range(start, stop):
        frames[t] = take(frames, d, t)
    return frames


def unfilled(cov_y, radius):
    """(T,) the number of positions of the Y (BGR: pixel) plane without a donor."""
    d = donors(cov_y, radius)
    return (d == NONE).reshape(d.shape[0], -1).sum(1)


def undecided(dist, delta, radius):
    """(T, h, w) bool: some frame within ``radius`` of t has the position within ``delta`` of a coverage threshold -- its coverage, and so
    the donor of frame t, may be decided either way by a coordinate that is ``delta`` off."""
    near = dist <= delta
    out = near.copy()
    n = near.shape[0]
    for k in range(1, radius + 1):
        out[k:] |= near[:n - k]
        out[:n - k] |= near[k:]
    return out


# ---------------------------------------------------------------- the inputs of tests/test_hip_mosaic.py (the CPU test checks their condition)
T, R = 9, 3
SHAPES, BIG = keep_ref.SHAPES, keep_ref.BIG
FIELDS = ["ramp", "ramp_zoom", "smooth", "identity"]


def field_case(case, size, seed):
    """(T, size, size, 2) float32.  "ramp": a shift that runs linearly over the clip, the wedge moving from two sides to the opposite two, so
    that every donor distance -R .. R and "none" occur; "ramp_zoom": the same zoomed out by 1.07, a rim on all sides; "smooth": yuv16_ref's
    smooth random field as keep_ref.field_case calls it (ragged rims); "identity": keep_ref's, every frame the same."""
    import yuv16_ref
    if case in ("ramp", "ramp_zoom"):
        scale = 1.07 if case == "ramp_zoom" else 1.0
        return np.concatenate([bicubic_ref.affine_field(1, size, size, scale=scale, shift=(0.33 * s + 0.0137, -0.21 * s - 0.0091))
                               for s in np.linspace(-1.0, 1.0, T)])
    if case == "identity":
        return np.repeat(keep_ref.field_case("identity", size, seed)[:1], T, 0)
    return yuv16_ref.smooth_field(T, seed, size=size) if size > 8 else yuv16_ref.smooth_field(T, seed, scale=1.3, size=size)
