"""numpy restatement of the scene-cut score and the per-scene window clamp (csrc/scene.hip, stream.scene_scores / find_scene_cuts /
VideoStabilizer._layout), written from the definitions only: what the GPU tests compare against, bit for bit."""
import numpy as np

GRID, BINS = 4, 32


def bins(planes):
    """bin of every sample: x = (v + 1) * 16 in fp32; 0 if not x >= 0 (NaN, below -1), else min(31, int(x))."""
    x = (np.asarray(planes, np.float32) + np.float32(1.0)) * np.float32(16.0)
    assert x.dtype == np.float32
    ok = x >= 0                                   # False for NaN
    with np.errstate(invalid="ignore"):
        xi = np.where(ok & (x < BINS), x, 0).astype(np.int64)      # truncation of values in [0, 32)
    return np.where(ok, np.where(x >= BINS, BINS - 1, xi), 0)


def hist(planes):
    """(n, h, w) -> (n, 16, 32) uint32: block by * 4 + bx of the 4 x 4 grid of (h/4) x (w/4) blocks."""
    planes = np.asarray(planes, np.float32)
    n, h, w = planes.shape
    assert h % GRID == 0 and w % GRID == 0
    bh, bw = h // GRID, w // GRID
    b = bins(planes)
    out = np.zeros((n, GRID * GRID, BINS), np.uint32)
    for t in range(n):
        for by in range(GRID):
            for bx in range(GRID):
                blk = b[t, by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw]
                out[t, by * GRID + bx] = np.bincount(blk.ravel(), minlength=BINS)
    return out


def sad(h):
    """(n, 16, 32) -> (n,) uint32: sad[0] = 0, sad[t] = sum |hist[t] - hist[t-1]|."""
    h = h.astype(np.int64).reshape(h.shape[0], -1)
    out = np.zeros(h.shape[0], np.uint32)
    out[1:] = np.abs(h[1:] - h[:-1]).sum(1)
    return out


def scores(planes):
    """(n,) float32 = sad / (2 h w): the exact integer rounded to fp32, divided in fp32 (correctly rounded; torch's division of a device
    tensor by a scalar gives the same bits when 2 h w is a power of two, as for 256 x 256 planes, and may differ by one ulp otherwise)."""
    planes = np.asarray(planes, np.float32)
    return sad(hist(planes)).astype(np.float32) / np.float32(2 * planes.shape[1] * planes.shape[2])


def find_cuts(score, threshold=0.25, min_scene=16):
    cuts, last = [], 0
    for t in range(1, len(score)):
        if score[t] > threshold and t - last >= min_scene:
            cuts.append(t)
            last = t
    return cuts


def windows_index(T, cuts, period=30):
    """(T, period + 1) table: plane j of frame i's window is gray[table[i, j]] = clamp(i - period//2 + j, a, b - 1) for i in scene [a, b)."""
    half = period // 2
    edges = [0] + list(cuts) + [T]
    out = np.zeros((T, period + 1), np.int64)
    for a, b in zip(edges[:-1], edges[1:]):
        for i in range(a, b):
            out[i] = np.clip(np.arange(i - half, i + half + 1), a, b - 1)
    return out
