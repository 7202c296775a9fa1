"""What a clip's fields leave of the frame: the per-frame homography fit and the host arithmetic of crop and zoom windows."""
import math

import torch

from . import hipabi as A
from .scenes import _cut_list, _scenes


def _field_homography(field, h0, w0, m_out, bounds_out, pts_out=None):
    A.check(A.lib().pws_field_homography(A.ptr(field), field.shape[0], field.shape[1], field.shape[2], h0, w0, A.ptr(m_out),
                                         A.ptr(bounds_out), A.ptr(pts_out), A.current_stream()), "pws_field_homography")


def _has_lattice(h0, w0):
    """Whether an h0 x w0 frame holds the homography fit's 20 x 20 sampling lattice."""
    return h0 >= 300 and w0 >= 600


def _check_lattice(h0, w0, what="automatic crop"):
    """``what``: the feature that asked for the fit, for the message."""
    if not _has_lattice(h0, w0):
        raise ValueError("%s: the homography fit's 20 x 20 sampling lattice needs a frame of at least 600 x 300 pixels, got %d x %d" % (what, w0, h0))


def field_homography(field, frame_hw, return_points=False):
    """The per-frame half of the reference's automatic crop (main_new.py:550-574) on the device: ``field`` (N, fh, fw, 2) as
    ``netG(window, False)`` returns it, ``frame_hw`` = (H0, W0) of the source frames it warps.  The field resized to H0 x W0 as the warp
    resizes it is sampled on a 20 x 20 lattice (p1), the homography M (m33 = 1) from p1 to the lattice's own positions in [-1, 1] is
    fitted in fp64 (least squares on the reprojection error: cv2.findHomography's result when every sample is an inlier), and the
    corners mapped through it give the frame's bounds in source pixels.  Returns M (N, 3, 3) float64 and bounds (N, 4) float32 = (top,
    bottom, left, right) [and p1 (N, 400, 2) float32], all on the device; a frame without a well-defined fit has NaN M and bounds."""
    A.require_cuda(field)
    if field.dim() != 4 or field.shape[3] != 2:
        raise ValueError("field_homography: field must be (N, fh, fw, 2), got %s" % (tuple(field.shape),))
    h0, w0 = int(frame_hw[0]), int(frame_hw[1])
    _check_lattice(h0, w0)
    field = field.contiguous()
    n = field.shape[0]
    m = torch.empty((n, 3, 3), device=field.device, dtype=torch.float64)
    bounds = torch.empty((n, 4), device=field.device, dtype=torch.float32)
    pts = torch.empty((n, 400, 2), device=field.device, dtype=torch.float32) if return_points else None
    _field_homography(field, h0, w0, m, bounds, pts)
    return (m, bounds, pts) if return_points else (m, bounds)


def _bounds_rows(bounds, what):
    """Per-frame bounds (a tensor on either side, an array or a sequence) as T rows of 4 floats."""
    if isinstance(bounds, torch.Tensor):
        bounds = bounds.detach().to("cpu", torch.float64).tolist()
    bounds = [[float(v) for v in row] for row in bounds]
    if any(len(row) != 4 for row in bounds):
        raise ValueError("%s: bounds must be (T, 4): top, bottom, left, right" % what)
    return bounds


def _centred_window(k, h, w):
    """The window (x0, x1, y0, y1) of the fraction k of an h x w frame around its centre (float64, in this order of operations)."""
    return (0.5 * w - 0.5 * k * w, 0.5 * w + 0.5 * k * w, 0.5 * h - 0.5 * k * h, 0.5 * h + 0.5 * k * h)


def auto_crop_window(bounds, frame_hw, output_hw=None, period=30, scene_cuts=None):
    """The reference's crop recurrence (main_new.py:575-603) over a clip's per-frame bounds (``field_homography``; (T, 4) top, bottom,
    left, right in source pixels, a tensor on either side or an array): the window starts at the whole H0 x W0 frame, and each frame i
    with period//2 < i < T - period//2 pulls every edge that lies outside the frame's bounds half way towards them, in float64.  Returns
    (x_start, x_end, y_start, y_end), scaled to ``output_hw`` = (height, width) of the output frame when given, for run_video's ``crop``.
    ValueError when a frame the recurrence reads has NaN bounds, or when the window is empty.
    scene_cuts (sorted indices at which a new scene starts): the reference's end rule holds per scene -- frame i of scene [a, b) is read only
    if a + period//2 < i < b - period//2, since the frames next to a cut see a clamped window as those at the clip's ends do -- and the one
    window is carried from scene to scene (one output size serves the whole clip)."""
    bounds = _bounds_rows(bounds, "auto_crop_window")
    h0, w0 = int(frame_hw[0]), int(frame_hw[1])
    T, half, rate = len(bounds), int(period) // 2, 0.5
    x0, x1, y0, y1 = 0.0, float(w0), 0.0, float(h0)
    for i in (i for a, b in _scenes(T, _cut_list(scene_cuts, T, "auto_crop_window")) for i in range(a + half + 1, b - half)):
        top, bottom, left, right = bounds[i]
        if not all(math.isfinite(v) for v in bounds[i]):
            raise ValueError("auto_crop_window: frame %d has no homography (bounds %r)" % (i, bounds[i]))
        if y0 < top:
            y0 += (top - y0) * rate
        if y1 > bottom:
            y1 -= (y1 - bottom) * rate
        if x0 < left:
            x0 += (left - x0) * rate
        if x1 > right:
            x1 -= (x1 - right) * rate
    if output_hw is not None:
        sy, sx = int(output_hw[0]) / h0, int(output_hw[1]) / w0
        x0, x1, y0, y1 = x0 * sx, x1 * sx, y0 * sy, y1 * sy
    if not (int(x1) > int(x0) and int(y1) > int(y0)):
        raise ValueError("auto_crop_window: the crop window x [%g, %g) y [%g, %g) is empty" % (x0, x1, y0, y1))
    return x0, x1, y0, y1


def zoom_window(window, frame_hw):
    """The largest window of the frame's aspect centred inside ``window`` = (x0, x1, y0, y1) (source-pixel edge coordinates, as
    ``auto_crop_window(..., output_hw=None)`` returns them): with k = min((x1 - x0) / W0, (y1 - y0) / H0) and the window's centre (cx, cy),
    (cx - k W0 / 2, cx + k W0 / 2, cy - k H0 / 2, cy + k H0 / 2), kept inside ``window`` against the last rounding.  Zooming the H0 x W0
    frame into it scales both axes alike (vid.stab's ``zoom``).  Host arithmetic, float64."""
    x0, x1, y0, y1 = (float(v) for v in window)
    h0, w0 = int(frame_hw[0]), int(frame_hw[1])
    if not (x1 > x0 and y1 > y0 and h0 > 0 and w0 > 0):
        raise ValueError("zoom_window: the window x [%g, %g) y [%g, %g) is empty" % (x0, x1, y0, y1))
    k = min((x1 - x0) / w0, (y1 - y0) / h0)
    cx, cy = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    return (max(x0, cx - 0.5 * k * w0), min(x1, cx + 0.5 * k * w0), max(y0, cy - 0.5 * k * h0), min(y1, cy + 0.5 * k * h0))


def zoom_schedule(bounds, frame_hw, speed=0.002, min_window=0.5, scene_cuts=None):
    """Per-frame zoom windows from a clip's per-frame bounds (``field_homography``; (T, 4) top, bottom, left, right in source pixels): vid.stab's
    ``optzoom=2``.  Every window is centred on the frame's centre and has the frame's aspect, window t = the fraction k[t] of the frame.
    Frame t asks for k_req[t] = min(1, 2 min(W0/2 - left, right - W0/2) / W0, 2 min(H0/2 - top, bottom - H0/2) / H0), the largest centred window
    inside its bounds; kc = max(k_req, min_window) (a frame that asks for more zoom than 1 / min_window keeps some wedge); inside each scene
    k[t] = min over s of kc[s] + speed |t - s|: the largest schedule that never exceeds kc and never changes by more than ``speed`` per frame
    (two linear sweeps).  scene_cuts: sorted indices at which a new scene starts; the schedule is free to jump there.  NaN bounds are a
    ValueError naming the frame.  Returns T windows (x0, x1, y0, y1) for ``zoom_fields`` / ``run(zoom=)``.  Host arithmetic, float64."""
    bounds = _bounds_rows(bounds, "zoom_schedule")
    h0, w0 = int(frame_hw[0]), int(frame_hw[1])
    speed, min_window = float(speed), float(min_window)
    if not (speed >= 0.0 and 0.0 < min_window <= 1.0):
        raise ValueError("zoom_schedule: speed must be >= 0 and min_window in (0, 1], got %r and %r" % (speed, min_window))
    T = len(bounds)
    kc = []
    for t, row in enumerate(bounds):
        if not all(math.isfinite(v) for v in row):
            raise ValueError("zoom_schedule: frame %d has no homography (bounds %r)" % (t, row))
        top, bottom, left, right = row
        k_req = min(1.0, 2.0 * min(0.5 * w0 - left, right - 0.5 * w0) / w0, 2.0 * min(0.5 * h0 - top, bottom - 0.5 * h0) / h0)
        kc.append(max(k_req, min_window))
    k = list(kc)
    for a, b in _scenes(T, _cut_list(scene_cuts, T, "zoom_schedule")):
        for t in range(a + 1, b):
            k[t] = min(k[t], k[t - 1] + speed)
        for t in range(b - 2, a - 1, -1):
            k[t] = min(k[t], k[t + 1] + speed)
    return [_centred_window(v, h0, w0) for v in k]
