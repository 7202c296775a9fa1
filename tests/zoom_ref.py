"""Float64 restatement of zoom to fill (functional.zoom_fields, csrc/field_zoom.hip), plus the same operation sequence evaluated in numpy
float32: the yardstick the GPU tests measure the kernel against (tests/test_hip_zoom.py).

Definition.  A window (x0, x1, y0, y1) of the H0 x W0 frame, in source-pixel EDGE coordinates (pixel k covers [k, k + 1)).  Node j of a field
row stands for output pixel x = j (W0-1)/(fw-1) (the warps resize the field with align_corners=True); the centre of that pixel, x + 0.5, maps
to x0 + (x + 0.5) Bx in the window, Bx = (x1 - x0) / W0, i.e. to pixel coordinate x0 + (x + 0.5) Bx - 0.5, which on the field's scale is
sx = Bx j + Ax, Ax = (x0 + 0.5 Bx - 0.5) (fw-1)/(W0-1).  The zoomed field's node takes the field there (clamped to the field, bilinear);
its VALUE still means a source position, which `coverage` un-normalises as the warps do."""
import numpy as np

FACTOR = 4      # the project's 4x rule: tolerances are 4 x the float32 restatement's own error
CAP = 0.01      # largest share of nodes that may lie within delta of a coverage threshold


def coefficients(windows, frame_hw, field_hw):
    """(T, 4) float64: Ax, Bx, Ay, By per window."""
    h0, w0 = frame_hw
    fh, fw = field_hw
    w = np.asarray(windows, np.float64).reshape(-1, 4)
    bx, by = (w[:, 1] - w[:, 0]) / w0, (w[:, 3] - w[:, 2]) / h0
    ax = (w[:, 0] + 0.5 * bx - 0.5) * (fw - 1) / (w0 - 1)
    ay = (w[:, 2] + 0.5 * by - 0.5) * (fh - 1) / (h0 - 1)
    return np.stack([ax, bx, ay, by], 1)


def _axis64(a, b, n):
    s = np.clip(b * np.arange(n, dtype=np.float64) + a, 0.0, n - 1.0)
    i0 = np.floor(s).astype(np.int64)
    return i0, i0 + (i0 < n - 1), s - i0


def zoom64(field, coef):
    """The zoomed fields in float64: field (T, fh, fw, 2), coef (T, 4) float64."""
    field = np.asarray(field, np.float64)
    out = np.empty_like(field)
    T, fh, fw, _ = field.shape
    for t in range(T):
        ax, bx, ay, by = (float(v) for v in coef[t])
        x0, x1, lx = _axis64(ax, bx, fw)
        y0, y1, ly = _axis64(ay, by, fh)
        lx, ly = lx[None, :, None], ly[:, None, None]
        F = field[t]
        top = (1 - lx) * F[y0][:, x0] + lx * F[y0][:, x1]
        bot = (1 - lx) * F[y1][:, x0] + lx * F[y1][:, x1]
        out[t] = (1 - ly) * top + ly * bot
    return out


def _fma32(a, b, c):
    """fma(a, b, c) on float32 arrays: the product of two float32 is exact in float64; the sum is rounded to float64, then to float32 (a double
    rounding that differs from the single one only on a float64 tie pattern: irrelevant for a yardstick)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _axis32(a, b, n):
    j = np.arange(n, dtype=np.float32)
    s = np.clip(_fma32(np.full(n, b, np.float32), j, np.full(n, a, np.float32)), np.float32(0), np.float32(n - 1))
    i0 = np.floor(s).astype(np.int64)
    l = (s - i0.astype(np.float32)).astype(np.float32)
    return i0, i0 + (i0 < n - 1), l, (np.float32(1) - l).astype(np.float32)


def zoom32(field, coef):
    """The kernel's operation sequence in numpy float32: coef rounded to float32 (as uploaded), sx = clamp(fma(Bx, j, Ax)), lx = sx - x0,
    hx = 1 - lx, warp_common.h's field_lerp: top = fma(lx, b, hx * a), bot = fma(lx, d, hx * c), fma(ly, bot, hy * top)."""
    field = np.asarray(field, np.float32)
    coef = np.asarray(coef, np.float64).astype(np.float32)
    out = np.empty_like(field)
    T, fh, fw, _ = field.shape
    for t in range(T):
        x0, x1, lx, hx = _axis32(coef[t, 0], coef[t, 1], fw)
        y0, y1, ly, hy = _axis32(coef[t, 2], coef[t, 3], fh)
        shape = (fh, fw, 2)
        lx, hx = np.broadcast_to(lx[None, :, None], shape), np.broadcast_to(hx[None, :, None], shape)
        ly, hy = np.broadcast_to(ly[:, None, None], shape), np.broadcast_to(hy[:, None, None], shape)
        F = field[t]
        top = _fma32(lx, F[y0][:, x1], hx * F[y0][:, x0])
        bot = _fma32(lx, F[y1][:, x1], hx * F[y1][:, x0])
        out[t] = _fma32(ly, bot, hy * top)
    return out


def unnormalize64(g, size, align_corners):
    g = np.asarray(g, np.float64)
    return (g + 1) / 2 * (size - 1) if align_corners else ((g + 1) * size - 1) / 2


def unnormalize32(g, size, align_corners):
    """warp_common.h's unnormalize: one fma with float32 constants."""
    g = np.asarray(g, np.float32)
    k = np.float32(0.5) * np.float32(size - 1 if align_corners else size)
    return _fma32(g, np.full(g.shape, k, np.float32), np.full(g.shape, np.float32(0.5) * np.float32(size - 1), np.float32))


def margin(mode):
    return {"bilinear": 0, "bicubic": 1}[mode]


def coverage(zoomed, frame_hw, align_corners, m):
    """(covered (T, fh, fw) bool, dist (T, fh, fw)): a node is covered iff m <= ix <= W0-1-m and m <= iy <= H0-1-m (NaN: not covered); dist is
    its distance to the nearest of the four thresholds (0 for NaN: never decided)."""
    h0, w0 = frame_hw
    ix, iy = unnormalize64(zoomed[..., 0], w0, align_corners), unnormalize64(zoomed[..., 1], h0, align_corners)
    with np.errstate(invalid="ignore"):
        cov = (ix >= m) & (ix <= w0 - 1 - m) & (iy >= m) & (iy <= h0 - 1 - m)
        dist = np.minimum(np.minimum(np.abs(ix - m), np.abs(ix - (w0 - 1 - m))), np.minimum(np.abs(iy - m), np.abs(iy - (h0 - 1 - m))))
    return cov, np.where(np.isnan(dist), 0.0, dist)


def count_bounds(field, coef, frame_hw, align_corners, m):
    """Per frame (lo, hi, undecided share): the count of uncovered nodes lies in [lo, hi] -- lo = nodes uncovered in float64 by more than
    delta, hi = lo + the nodes within delta of a threshold; delta = FACTOR x the largest distance between the float32 sequence's coordinates
    (zoom32, unnormalize32) and the float64 ones on this very field."""
    h0, w0 = frame_hw
    z64, z32 = zoom64(field, coef), zoom32(field, coef)
    cov, dist = coverage(z64, frame_hw, align_corners, m)
    ex = np.abs(unnormalize32(z32[..., 0], w0, align_corners).astype(np.float64) - unnormalize64(z64[..., 0], w0, align_corners))
    ey = np.abs(unnormalize32(z32[..., 1], h0, align_corners).astype(np.float64) - unnormalize64(z64[..., 1], h0, align_corners))
    delta = FACTOR * max(float(ex.max()), float(ey.max()))
    decided = dist > delta
    lo = (~cov & decided).reshape(cov.shape[0], -1).sum(1)
    und = (~decided).reshape(cov.shape[0], -1).sum(1)
    return lo, lo + und, float((~decided).mean()), delta


def make_field(shape, seed, scale=1.0, noise=0.03):
    """(T, fh, fw, 2) float32: the identity grid in [-1, 1] x ``scale``, plus a smooth perturbation, plus ``noise`` of uniform noise."""
    T, fh, fw, _ = shape
    rs = np.random.RandomState(seed)
    u, v = np.meshgrid(np.linspace(-1, 1, fw), np.linspace(-1, 1, fh))
    out = np.empty(shape, np.float64)
    for t in range(T):
        p = rs.uniform(0, 2 * np.pi, 2)
        out[t, ..., 0] = scale * u + 0.05 * np.sin(np.pi * u + p[0]) * np.cos(0.5 * np.pi * v)
        out[t, ..., 1] = scale * v + 0.05 * np.cos(np.pi * v + p[1]) * np.sin(0.7 * np.pi * u)
    out += noise * rs.uniform(-1, 1, shape)
    return out.astype(np.float32)


def make_windows(T, frame_hw, seed):
    """T windows that differ per frame: the whole frame first, the centred half (k = 0.5) second, then off-centre fractional ones."""
    h0, w0 = frame_hw
    rs = np.random.RandomState(seed)
    wins = [(0.0, float(w0), 0.0, float(h0)), (0.25 * w0, 0.75 * w0, 0.25 * h0, 0.75 * h0)]
    while len(wins) < T:
        x0, y0 = rs.uniform(0, 0.3 * w0), rs.uniform(0, 0.3 * h0)
        wins.append((x0, x0 + rs.uniform(0.4, 0.7) * w0, y0, y0 + rs.uniform(0.4, 0.7) * h0))
    return wins[:T]


# the cases of tests/test_hip_zoom.py, shared with the CPU test that holds the reference's own undecided share under CAP
FRAME = (360, 640)
SHAPES = [(3, 256, 256, 2), (2, 24, 40, 2), (1, 2, 2, 2), (5, 67, 129, 2)]
COVER_SCALE = 1.04   # the identity grid scaled so that a band of nodes samples outside the source


def seed_of(shape):
    return shape[1] * 7 + shape[2]


def window_rounds(shape):
    """Lists of T windows: every shape sees the whole frame, the centred half and off-centre fractional windows, whatever its T."""
    T = shape[0]
    wins = make_windows(max(T, 4), FRAME, seed_of(shape))
    return [[wins[(r * T + t) % len(wins)] for t in range(T)] for r in range(-(-len(wins) // T))]
