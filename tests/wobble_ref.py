"""Float64 restatement of wobble suppression (functional.wobble_fields, csrc/field_wobble.hip), plus the same operation sequence with the
residual, the sums and the division in numpy float32: the yardstick the GPU tests measure the kernel against (tests/test_hip_wobble.py).

Definition.  One call is one scene of n frames: field (n, fh, fw, 2) float32, M (n, 9) float64 as field_homography fits it, the frame
(H0, W0), sigma in (0, 5] frames.  R = ceil(3 sigma) <= 15; g_k = exp(-k^2 / (2 sigma^2)), k = -R .. R, in float64, each rounded to float32
(g_0 = 1).  P[t] at node (i, j), a FITTED frame and a VALID node are rigid mode's, word for word (tests/rigid_ref.py `positions`): the
adjugate in float64, D/Dc >= 2^-20, P rounded once to float32.  A (frame, node) pair is USABLE when the frame is fitted, the node is valid
and both components of F are finite; then E = F - P.  A node that is not usable at t keeps F bit for bit and counts in unfit[t].  A usable
one becomes P[t] + S / W with S = sum g_k E[t+k] and W = sum g_k over the k, ascending, with 0 <= t+k < n and (t+k, node) usable: frames
outside the scene and unusable taps drop out of both sums -- no reflection, no padding; W >= 1 because k = 0 counts.  removed[t] = the largest
max(|out_x - F_x| W0/2, |out_y - F_y| H0/2) over the usable nodes of t (a NaN drops out), 0 without any: how far the filter moved the field, in
source pixels."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rigid_ref as G  # noqa: E402
import zoom_ref as Z  # noqa: E402

FACTOR = G.FACTOR   # the project's 4x rule
FRAME = G.FRAME
MAX_SIGMA = 5.0
SEGMENT = 32        # the kernel's time segment L (include/pwstable.h PWS_WOBBLE_SEGMENT, functional.WOBBLE_SEGMENT)
SIGMAS = (0.5, 2.0, 5.0)
# the cases of tests/test_hip_wobble.py, (n, fh, fw): one frame and odd width; n < R; the stabiliser's lattice, two segments; and n = L-1, L,
# L+1 and 2L+1 around the kernel's segment length at a width of two column chunks, the second one partial
SHAPES = [(1, 67, 129), (3, 67, 129), (40, 256, 256)] + [(n, 64, 130) for n in (SEGMENT - 1, SEGMENT, SEGMENT + 1, 2 * SEGMENT + 1)]


def seed_of(shape):
    return shape[0] * 131 + shape[1] * 7 + shape[2]


def radius(sigma):
    return int(math.ceil(3.0 * float(sigma)))


def weights(sigma):
    """g_k, k = -R .. R: float64 on the host, rounded to float32."""
    k = np.arange(-radius(sigma), radius(sigma) + 1, dtype=np.float64)
    return np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma))).astype(np.float32)


def parts(field, m, frame_hw):
    """(P32 (n, fh, fw, 2) float32, usable (n, fh, fw) bool) of a scene: rigid_ref.positions per frame, P rounded once."""
    field = np.asarray(field, np.float32)
    n, fh, fw, _ = field.shape
    m = np.asarray(m, np.float64).reshape(n, 9)
    P32, usable = np.empty_like(field), np.empty((n, fh, fw), bool)
    for t in range(n):
        P, valid, _ = G.positions(m[t], (fh, fw), frame_hw)
        with np.errstate(all="ignore"):
            P32[t] = P.astype(np.float32)
        usable[t] = valid & np.isfinite(field[t]).all(-1)
    return P32, usable


def _taps(n, k):
    """(destination slice, source slice) of tap k: the frames t with 0 <= t + k < n, and t + k."""
    return slice(max(0, -k), n - max(0, k)), slice(max(0, k), n + min(0, k))


def _removed(absdiff, usable, frame_hw):
    h0, w0 = frame_hw
    d = (absdiff * np.array([w0 / 2, h0 / 2], absdiff.dtype)).max(-1)
    d = np.where(np.isnan(d) | ~usable, absdiff.dtype.type(0), d)
    return d.reshape(d.shape[0], -1).max(1)


def wobble64(field, m, frame_hw, sigma, parts_=None):
    """(out (n, fh, fw, 2) float64, removed (n,) float64, unfit (n,) int64): the definition in float64, with P and the weights rounded to
    float32 as defined."""
    field = np.asarray(field, np.float32)
    n = field.shape[0]
    P32, usable = parts_ if parts_ is not None else parts(field, m, frame_hw)
    F, P = field.astype(np.float64), P32.astype(np.float64)
    g, R = weights(sigma).astype(np.float64), radius(sigma)
    with np.errstate(all="ignore"):
        E = np.where(usable[..., None], F - P, 0.0)
        S, W = np.zeros_like(E), np.zeros(usable.shape)
        for k in range(-R, R + 1):
            dst, src = _taps(n, k)
            if dst.start < dst.stop:
                S[dst] += g[k + R] * E[src]
                W[dst] += g[k + R] * usable[src]
        out = np.where(usable[..., None], P + S / np.where(usable, W, 1.0)[..., None], F)
        removed = _removed(np.abs(out - F), usable, frame_hw)
    return out, removed, (~usable).reshape(n, -1).sum(1).astype(np.int64)


def wobble32(field, m, frame_hw, sigma, parts_=None):
    """The kernel's operation sequence with the float32 part in numpy float32: E = F - P (one subtraction), S by fma(g_k, E, S) from 0 in
    ascending k (Z._fma32; an unusable tap holds E = 0, which leaves S as it is), W by float32 additions, out = P + S / W (one division, one
    addition), removed from |out - F| (one subtraction) times the float32 W0/2 or H0/2.  (out float32, removed (n,) float32, unfit)."""
    field = np.asarray(field, np.float32)
    n = field.shape[0]
    P32, usable = parts_ if parts_ is not None else parts(field, m, frame_hw)
    g, R = weights(sigma), radius(sigma)
    with np.errstate(all="ignore"):
        E = np.where(usable[..., None], (field - P32).astype(np.float32), np.float32(0))
        S, W = np.zeros_like(E), np.zeros(usable.shape, np.float32)
        for k in range(-R, R + 1):
            dst, src = _taps(n, k)
            if dst.start < dst.stop:
                S[dst] = Z._fma32(np.full(E[src].shape, g[k + R], np.float32), E[src], S[dst])
                W[dst] = (W[dst] + np.where(usable[src], g[k + R], np.float32(0))).astype(np.float32)
        q = (S / np.where(usable, W, np.float32(1))[..., None]).astype(np.float32)
        out = np.where(usable[..., None], (P32 + q).astype(np.float32), field)
        removed = _removed(np.abs(out - field).astype(np.float32), usable, frame_hw)
    return out, removed.astype(np.float32), (~usable).reshape(n, -1).sum(1).astype(np.int64)


def scenes(n, cuts):
    edges = [0] + [int(c) for c in (cuts or [])] + [n]
    return list(zip(edges[:-1], edges[1:]))


def wobble64_scenes(field, m, frame_hw, sigma, cuts):
    """wobble64 scene by scene: taps never cross a cut."""
    field, m = np.asarray(field, np.float32), np.asarray(m, np.float64).reshape(len(field), 9)
    res = [wobble64(field[a:b], m[a:b], frame_hw, sigma) for a, b in scenes(len(field), cuts)]
    return tuple(np.concatenate([r[i] for r in res]) for i in range(3))


def removed_error_px(field, m, frame_hw, sigma, parts_=None, outs=None):
    """The float32 sequence's own error in `removed`'s per-node distance, in source pixels (rigid_ref.coordinate_error_px's construction):
    the largest difference, over the usable nodes, between max(|out - F| (W0/2, H0/2)) of wobble32 and of wobble64, plus the share P's own
    float32 rounding has in it, half an ulp of the largest finite |P| times max(W0, H0)/2.  ``outs`` = (wobble64's out, wobble32's out) when
    the caller has them."""
    field = np.asarray(field, np.float32)
    h0, w0 = frame_hw
    parts_ = parts_ if parts_ is not None else parts(field, m, frame_hw)
    P32, usable = parts_
    if not usable.any():
        return 0.0
    o64, o32 = outs if outs is not None else (wobble64(field, m, frame_hw, sigma, parts_)[0], wobble32(field, m, frame_hw, sigma, parts_)[0])
    with np.errstate(all="ignore"):
        d64 = (np.abs(o64 - field) * np.array([w0 / 2, h0 / 2])).max(-1)
        d32 = (np.abs(o32 - field).astype(np.float32) * np.array([w0 / 2, h0 / 2], np.float32)).max(-1).astype(np.float64)
        diff = np.abs(d32 - d64)[usable]
    pmax = np.abs(P32[usable])
    pmax = float(pmax[np.isfinite(pmax)].max()) if np.isfinite(pmax).any() else 0.0
    return float(np.nanmax(diff)) + 0.5 * float(np.spacing(np.float32(pmax))) * max(w0, h0) / 2


def make_inputs(shape, seed=None):
    """(field (n, fh, fw, 2) float32, m (n, 9) float64) of one case: rigid mode's fields -- the identity grid plus a smooth perturbation plus
    3 % noise, new in every frame -- and a different homography per frame."""
    n, fh, fw = shape
    seed = seed_of(shape) if seed is None else seed
    return G.make_field((n, fh, fw, 2), seed), G.make_homographies(n, seed)


def wobbly_clip(n, field_hw, frame_hw, amplitude, seed):
    """A synthetic clip's fields with injected wobble: field[t] = the exact field of a smooth homography path + a static smooth distortion
    + white per-frame, per-node noise of RMS ``amplitude`` (normalised units).  Returns (field float32, m (n, 9) float64 -- the path's
    homographies, which the tests use as the fit --, the noise (n, fh, fw, 2) float64)."""
    rs = np.random.RandomState(seed)
    fh, fw = field_hw
    u, v = G.node_uv(field_hw, frame_hw)
    static = 0.01 * np.stack([np.sin(2.5 * v)[:, None] * np.cos(1.5 * u)[None, :], np.cos(2.0 * u)[None, :] * np.sin(3.0 * v)[:, None]], -1)
    m = np.empty((n, 9))
    field = np.empty((n, fh, fw, 2), np.float64)
    for t in range(n):
        a, s = np.deg2rad(1.5 * np.sin(0.11 * t)), 1 + 0.02 * np.cos(0.07 * t)
        m[t] = [s * np.cos(a), -s * np.sin(a), 0.03 * np.sin(0.05 * t), s * np.sin(a), s * np.cos(a), 0.02 * np.cos(0.09 * t), 0.005, -0.004, 1.0]
        field[t] = G.field_from_homography(m[t], field_hw, frame_hw).astype(np.float64) + static
    noise = rs.standard_normal(field.shape) * amplitude
    return (field + noise).astype(np.float32), m, noise


def expected_attenuation(sigma):
    """sqrt(sum g^2) / sum g: what the filter leaves of white noise at an interior frame."""
    g = weights(sigma).astype(np.float64)
    return float(np.sqrt((g * g).sum()) / g.sum())
