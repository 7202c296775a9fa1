"""Streaming video stabilisation: the device-side counterpart of the reference's ``process()`` loop
(reference main_new.py:612-741) minus its OpenCV I/O (decode, BGR->gray, INTER_AREA resize, MJPG encode stay with the
caller -- cv2 is not part of the accelerated path).

Per frame i the reference builds a 31-frame window of 256x256 gray frames [i-15, i+15] (the first / last frame
repeated at the ends, main_new.py:627-633,653-660), runs ``netG(window, False)``, resizes the 256x256 field to the frame
size (UpsamplingBilinear2d) and warps the full-resolution RGB frame (grid_sample), one frame at a time with a
host<->device round trip per frame.  Here:
  * frames are processed in batches of ``batch`` windows per generator call (the windows are overlapping views of one
    gray-frame buffer, gathered on the device);
  * field resize + warp is the fused HIP kernel (the resized field is never materialised);
  * when the inputs live in (pinned) host memory, batch k+1 is copied H2D on a side stream while batch k computes,
    and results go D2H on a third stream (hipMemcpyAsync through torch, one event per hand-off);
  * several GPUs take contiguous frame chunks with a 15-frame halo each (``distributed.shard_frames``): no collective.
"""
import math
import time

import torch

from . import functional as PF
from . import hipabi as A


def _window_planes(frames, fmt, size, out, what, frames_are_rgb=False):
    """The window planes of frames in the format ``fmt`` (functional.FrameFormat) in one launch: what window_planes, window_planes_yuv and
    window_planes_yuv16 document.  The format's shape rules (ValueError, width a multiple of 2) come before host tensors or a wrong dtype."""
    t, h, w = fmt.frame_shape(frames, w_multiple=2)
    A.require_cuda(frames, dtype=fmt.dtype)
    if fmt.hwc and frames.shape[3] != 3:
        raise ValueError("%s: frames must be (T, H, W, 3) uint8, got %s" % (what, tuple(frames.shape),))
    frames = frames.contiguous()
    if out is None:
        out = torch.empty((t, size, size), device=frames.device, dtype=torch.float32)
    A.require_cuda(out)
    if tuple(out.shape) != (t, size, size) or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous (T, %d, %d) float32 tensor" % (what, size, size))
    A.check(getattr(A.lib(), fmt.window_planes)(A.ptr(frames), A.ptr(out), t, h, w, size, size, 1, *fmt.args(frames_are_rgb), A.current_stream()),
            fmt.window_planes)
    return out


def window_planes(frames_hwc, size=256, frames_are_rgb=False, out=None):
    """``cv2.resize(cv2.cvtColor(frame, COLOR_BGR2GRAY), (size, size), INTER_AREA) / 255 * 2 - 1`` for a batch of decoded
    frames (reference main_new.py:639-643,653-667) on the device: (T, H, W, 3) uint8 -> (T, size, size) float32."""
    A.require_cuda(frames_hwc, dtype=torch.uint8)
    if frames_hwc.dim() != 4:
        raise ValueError("window_planes: frames must be (T, H, W, 3) uint8, got %s" % (tuple(frames_hwc.shape),))
    return _window_planes(frames_hwc, PF.FRAME_FORMATS["bgr24"], size, out, "window_planes", frames_are_rgb)


def area_half(frames_hwc, swap_rb=False):
    """``cv2.cvtColor(cv2.resize(frame, (W/2, H/2), INTER_AREA), COLOR_BGR2RGB)`` of the output frames (main_new.py:723-725;
    the swap is optional): (T, H, W, 3) uint8 -> (T, H/2, W/2, 3) uint8."""
    A.require_cuda(frames_hwc, dtype=torch.uint8)
    frames_hwc = frames_hwc.contiguous()
    t, h, w, _ = frames_hwc.shape
    out = torch.empty((t, h // 2, w // 2, 3), device=frames_hwc.device, dtype=torch.uint8)
    A.check(A.lib().pws_area_half_u8(A.ptr(frames_hwc), A.ptr(out), t, h, w, int(bool(swap_rb)), A.current_stream()),
            "pws_area_half_u8")
    return out


def area_resize(frames_hwc, size, swap_rb=False):
    """``cv2.resize(frame, size, interpolation=cv2.INTER_AREA)`` for any down-scaling ratio, ``size`` = (width, height) as cv2 takes
    it (main_new.py:723: ``cv2.resize(samples, (640, 360), interpolation=cv2.INTER_AREA)``): (T, H, W, 3) uint8 -> (T, height, width, 3)."""
    A.require_cuda(frames_hwc, dtype=torch.uint8)
    frames_hwc = frames_hwc.contiguous()
    t, h, w, _ = frames_hwc.shape
    ow, oh = int(size[0]), int(size[1])
    out = torch.empty((t, oh, ow, 3), device=frames_hwc.device, dtype=torch.uint8)
    A.check(A.lib().pws_area_resize_u8(A.ptr(frames_hwc), A.ptr(out), t, h, w, oh, ow, int(bool(swap_rb)), A.current_stream()),
            "pws_area_resize_u8")
    return out


def window_planes_yuv(frames, pixel_format, size=256, out=None):
    """window_planes of the BGR frames ``cv2.cvtColor(frame, COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_I420)`` would give, straight from packed
    4:2:0 frames (T, H * 3 // 2, W) uint8 in one launch (BT.601 limited range, OpenCV 4.x's 8-bit fixed point): the same planes bit for
    bit, so a YUV clip gets the fields of its BGR decode.  H and W even.  -> (T, size, size) float32."""
    A.require_cuda(frames, dtype=torch.uint8)   # (wins over the format's name and shape rules here, as it always has)
    return _window_planes(frames, _yuv_format(pixel_format, torch.uint8), size, out, "window_planes_yuv")


def _yuv_format(pixel_format, dtype):
    """The record of a packed YUV format of that sample dtype: a 4:2:0 name, or -- the 4:2:0 wrappers' ValueError for any other name staying
    word for word -- one of the 4:2:2 / 4:4:4 names of functional.CHROMA_FORMATS."""
    fmt = PF.lookup_format(pixel_format)
    if fmt is not None and fmt.packed and fmt.dtype == dtype:
        return fmt
    return PF._packed_format(pixel_format, dtype)


def _yuv_planes(x, h, w, pixel_format):
    """Views of the planes of packed frames x (T, packed rows of h, w) (FrameFormat.planes): [Y (T, h, w), UV (T, h/2, w)] for NV12, [Y, U
    (T, h/2, w/2), V (T, h/2, w/2)] for I420; P010 as NV12 and I010 as I420, in 16-bit words; chroma planes of h x w/2 for the 4:2:2 formats
    and h x w for 4:4:4."""
    return PF.lookup_format(pixel_format).planes(x, h, w)


def _area_resize_yuv(frames, fmt, size, what):
    """INTER_AREA plane by plane for packed frames in the format ``fmt``: what area_resize_yuv and area_resize_yuv16 document.  The output
    size is a multiple of the format's subsampling per axis (4:2:0: both even; 4:2:2: the width; 4:4:4: free)."""
    t, h, w = fmt.frame_shape(frames, w_multiple=2)
    A.require_cuda(frames, dtype=fmt.dtype)
    ow, oh = int(size[0]), int(size[1])
    (cx, cy), (mx, my) = fmt.shifts, fmt.multiples
    if ow % mx or oh % my or not (0 < ow <= w and 0 < oh <= h):
        if fmt.chroma == 0:
            raise ValueError("%s: output size %s must be even and within the %d x %d source" % (what, tuple(size), w, h))
        raise ValueError("%s: %s output size %s must be a multiple of %d x %d and within the %d x %d source" % (what, fmt.name, tuple(size), mx, my, w, h))
    frames = frames.contiguous()
    out = torch.empty(_frames_shape(fmt, t, oh, ow), device=frames.device, dtype=fmt.dtype)
    fs, os_ = frames[0].numel(), out[0].numel()   # (in samples)
    ch_, cw_, qh_, qw_ = h >> cy, w >> cx, oh >> cy, ow >> cx   # the chroma planes, source and output
    geo = [(1, h, w, oh, ow)] + ([(2, ch_, cw_, qh_, qw_)] if fmt.layout == 0 else [(1, ch_, cw_, qh_, qw_)] * 2)
    placement = (fmt.layout,) if fmt.dtype == torch.uint16 else ()   # (the 16-bit entry also takes where the 10 bits sit in a word)
    for (c, ph, pw, qh, qw), src, dst in zip(geo, _yuv_planes(frames, h, w, fmt.name), _yuv_planes(out, oh, ow, fmt.name)):
        A.check(getattr(A.lib(), fmt.plane_resize)(A.ptr(src), fs, A.ptr(dst), os_, t, ph, pw, c, qh, qw, *placement, A.current_stream()),
                fmt.plane_resize)
    return out


def area_resize_yuv(frames, pixel_format, size):
    """area_resize for packed 4:2:0 frames, plane by plane: Y to (height, width), the chroma to (height/2, width/2) (NV12's interleaved UV
    as a 2-channel image, I420's U and V as 1-channel images); ``size`` = (width, height), both even.  (T, H * 3 // 2, W) uint8 ->
    (T, height * 3 // 2, width)."""
    A.require_cuda(frames, dtype=torch.uint8)   # (wins over the format's name and shape rules here, as it always has)
    return _area_resize_yuv(frames, _yuv_format(pixel_format, torch.uint8), size, "area_resize_yuv")


def window_planes_yuv16(frames, pixel_format, size=256, out=None):
    """window_planes_yuv for 10-bit frames (T, H * 3 // 2, W) uint16, "p010" or "i010": the generator was trained on 8-bit gray, so the plane
    of a 10-bit frame is by definition the plane of its 8-bit reduction ``v8 = min(255, (v10 + 2) >> 2)``, fused into the kernel's loads (no
    8-bit copy of the frames): a P010 / I010 clip gets the fields of the NV12 / I420 clip of its reduced samples bit for bit.  H and W even.
    -> (T, size, size) float32."""
    return _window_planes(frames, _yuv_format(pixel_format, torch.uint16), size, out, "window_planes_yuv16")


def area_resize_yuv16(frames, pixel_format, size):
    """area_resize_yuv for 10-bit frames, INTER_AREA plane by plane on the 10-bit values (P010's interleaved UV as a 2-channel image),
    clamped to 0..1023 and stored in the format's placement; ``size`` = (width, height), both even.  (T, H * 3 // 2, W) uint16 ->
    (T, height * 3 // 2, width)."""
    return _area_resize_yuv(frames, _yuv_format(pixel_format, torch.uint16), size, "area_resize_yuv16")


def _yuv_crop(x, h, w, pixel_format, cy0, cy1, cx0, cx1):
    """The window [cy0, cy1) x [cx0, cx1) of packed frames (edges: multiples of the format's subsampling per axis -- even for 4:2:0), packed
    again on the device: Y [cy0:cy1, cx0:cx1], chroma [cy0 >> cy:cy1 >> cy, cx0 >> cx:cx1 >> cx]."""
    fmt = PF.lookup_format(pixel_format)
    cx, cy = fmt.shifts
    ch, cw = cy1 - cy0, cx1 - cx0
    out = torch.empty(_frames_shape(fmt, x.shape[0], ch, cw), device=x.device, dtype=x.dtype)
    src, dst = fmt.planes(x, h, w), fmt.planes(out, ch, cw)
    dst[0].copy_(src[0][:, cy0:cy1, cx0:cx1])
    if len(src) == 2:
        dst[1].copy_(src[1][:, cy0 >> cy:cy1 >> cy, cx0:cx1])   # (U V interleaved, cx = 1: chroma columns cx0/2 .. are samples cx0 ..)
    else:
        for k in (1, 2):
            dst[k].copy_(src[k][:, cy0 >> cy:cy1 >> cy, cx0 >> cx:cx1 >> cx])
    return out


def _output_resize(frames, fmt, size, half):
    """run_video's resize of warped frames to ``size`` = (width, height); half: BGR's 2 x 2 kernel (the YUV planes take the general one)."""
    if fmt.packed:
        return _area_resize_yuv(frames, fmt, size, "run_video")
    return area_half(frames) if half else area_resize(frames, size)


def _frames_shape(fmt, n, h, w):
    """The shape of n integer frames of h x w pixels in the format ``fmt``."""
    return (n, fmt.packed_rows(h), w) if fmt.packed else (n, h, w, 3)


def _crop(frames, fmt, h, w, cy0, cy1, cx0, cx1):
    """The window [cy0, cy1) x [cx0, cx1) of h x w frames, packed on the device: only the window crosses PCIe."""
    return _yuv_crop(frames, h, w, fmt.name, cy0, cy1, cx0, cx1) if fmt.packed else frames[:, cy0:cy1, cx0:cx1, :].contiguous()


def _prefetch(frames, s, e, stream, dev):
    """frames[s:e] on the device and the event to wait for: device-resident frames are read in place (no event), host frames go up on ``stream``."""
    if frames.is_cuda:
        return frames[s:e], None
    with torch.cuda.stream(stream):
        buf = frames[s:e].to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
    return buf, ev


def _field_homography(field, h0, w0, m_out, bounds_out, pts_out=None):
    A.check(A.lib().pws_field_homography(A.ptr(field), field.shape[0], field.shape[1], field.shape[2], h0, w0, A.ptr(m_out),
                                         A.ptr(bounds_out), A.ptr(pts_out), A.current_stream()), "pws_field_homography")


def _check_lattice(h0, w0, what="automatic crop"):
    """``what``: the feature that asked for the fit, for the message."""
    if h0 < 300 or w0 < 600:
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


def scene_scores(planes, return_counts=False):
    """The cut score of consecutive window planes (csrc/scene.hip): ``planes`` (T, h, w) float32 on the device, contiguous, h and w
    multiples of 4 (``window_planes``: 256 x 256).  Every plane is summarised by the 32-bin histograms of its 4 x 4 blocks (512 counters; the
    bin of a sample v is ``min(31, int((v + 1) * 16))``, 0 below -1 and for NaN); ``score[t] = sum |hist[t] - hist[t-1]| / (2 h w)`` lies in
    [0, 1] (0: the same block histograms, which a shaky shot nearly keeps; 1: no sample of any block kept its bin), ``score[0] = 0``.  The
    counters are exact integers and the division is torch's on them: the same bits on every run.  Returns (T,) float32 on the device
    [, hist (T, 16, 32) int32, sad (T,) int32].  A tensor that is not contiguous float32 (T, h, w) is a ValueError."""
    if not isinstance(planes, torch.Tensor) or planes.dim() != 3 or planes.dtype != torch.float32 or not planes.is_contiguous():
        raise ValueError("scene_scores: planes must be a contiguous (T, h, w) float32 tensor")
    A.require_cuda(planes)
    t, h, w = planes.shape
    hist = torch.empty((t, 16, 32), device=planes.device, dtype=torch.int32)
    sad = torch.empty((t,), device=planes.device, dtype=torch.int32)
    A.check(A.lib().pws_scene_change(A.ptr(planes), t, h, w, A.ptr(hist), A.ptr(sad), A.current_stream()), "pws_scene_change")
    scores = sad.to(torch.float32) / float(2 * h * w)
    return (scores, hist, sad) if return_counts else scores


def _motion_planes(planes, radius, what):
    if not isinstance(planes, torch.Tensor) or planes.dim() != 3 or planes.dtype != torch.float32 or not planes.is_contiguous():
        raise ValueError("%s: planes must be a contiguous (T, h, w) float32 tensor" % what)
    A.require_cuda(planes)
    radius = int(radius)
    t, h, w = planes.shape
    if not 1 <= radius <= 16:
        raise ValueError("%s: radius must be 1 .. 16, got %r" % (what, radius))
    if h - 2 * radius < 16 or w - 2 * radius < 16:
        raise ValueError("%s: a %d x %d plane holds no 16 x 16 block inside a margin of %d" % (what, h, w, radius))
    return t, h, w, radius


def block_motion(planes, radius=16):
    """Block motion between consecutive window planes (csrc/motion.hip; include/pwstable.h pws_block_motion has the definition): ``planes``
    (T, h, w) float32 on the device, contiguous (``window_planes``: 256 x 256, 14 x 14 blocks at the default radius).  The samples are
    quantised to bytes once; every 16 x 16 block of frame t is searched in frame t-1 over dx, dy in [-radius, radius] by its sum of absolute
    differences, ties going to the shorter vector.  Returns mv (T, nby, nbx, 2) int16 = (dx, dy), sad (T, nby, nbx, 5) int32 (the best
    candidate's and its four neighbours', -1 outside the range) and activity (T, nby, nbx) int32 (the block's summed absolute gradients),
    on the device; row 0 of mv and sad is zero.  Integer arithmetic after the quantisation: the same bits on every run.  A tensor that is
    not contiguous float32 (T, h, w), a radius outside 1 .. 16 or a plane without a block is a ValueError."""
    t, h, w, radius = _motion_planes(planes, radius, "block_motion")
    nby, nbx = (h - 2 * radius) // 16, (w - 2 * radius) // 16
    mv = torch.empty((t, nby, nbx, 2), device=planes.device, dtype=torch.int16)
    sad = torch.empty((t, nby, nbx, 5), device=planes.device, dtype=torch.int32)
    act = torch.empty((t, nby, nbx), device=planes.device, dtype=torch.int32)
    A.check(A.lib().pws_block_motion(A.ptr(planes), t, h, w, radius, A.ptr(mv), A.ptr(sad), A.ptr(act), A.current_stream()), "pws_block_motion")
    return mv, sad, act


def _check_pixel_scale(pixel_scale, what):
    """``pixel_scale`` as (sx, sy), two floats in (0, 1e6]; ValueError otherwise (NaN included)."""
    try:
        sx, sy = (float(v) for v in pixel_scale)
    except (TypeError, ValueError):
        raise ValueError("%s: pixel_scale must be None or (sx, sy), got %r" % (what, pixel_scale)) from None
    if not (0.0 < sx <= 1e6 and 0.0 < sy <= 1e6):
        raise ValueError("%s: pixel_scale must be two positive finite numbers, got %r" % (what, pixel_scale))
    return sx, sy


def global_motion(planes, radius=16, min_activity=2000, return_blocks=False, pixel_scale=None):
    """The similarity between consecutive window planes: ``block_motion``, then per pair the least-squares fit, in fp64, of ``p' = [[a, -b],
    [b, a]] p + (tx, ty)`` -- a block centre p of frame t, relative to the plane centre, lies at p' in frame t-1 -- to the blocks' sub-pixel
    vectors, in three rounds that drop outliers (pws_motion_fit has the definition).  A block counts if its activity is at least
    ``min_activity``, its vector lies inside the search range and its match is sharp (S rises around it by at least half the activity: a
    block whose content has left the search window settles on a chance match, around which S is flat).  The default 2000 is a judgement: a flat block measures 0, the blocks of the
    tests' synthetic texture a few thousand, and no real footage was available to fit the value to.  Returns motion (T, 4) float64 = (a, b,
    tx, ty) in plane pixels and inliers (T,) int32 [, mv, sad, activity], all on the device, no synchronisation; row 0 is (1, 0, 0, 0) with
    0 inliers, and a pair with fewer than 8 usable blocks in any round is a NaN row with 0 inliers.  Fixed summation order: the same bits on
    every run.  ValueError as for ``block_motion``.
    pixel_scale = (sx, sy): frame pixels per plane pixel, (W0 / w, H0 / h).  The planes are a non-uniform resize of any frame that is not
    square, under which a frame's rotation is no similarity; the fit then runs in FRAME pixels, relative to the frame centre
    (pws_motion_fit_scaled: centres and vectors scaled before the sums, the outlier floor sx sy), and so does the returned motion.  None,
    the default, is the plane-pixel fit as it was, which (1, 1) equals bit for bit; anything but two positive finite numbers is a
    ValueError."""
    t, h, w, radius = _motion_planes(planes, radius, "global_motion")
    if pixel_scale is not None:
        sx, sy = _check_pixel_scale(pixel_scale, "global_motion")
    mv, sad, act = block_motion(planes, radius)
    motion = torch.empty((t, 4), device=planes.device, dtype=torch.float64)
    inliers = torch.empty((t,), device=planes.device, dtype=torch.int32)
    if pixel_scale is None:
        A.check(A.lib().pws_motion_fit(A.ptr(mv), A.ptr(sad), A.ptr(act), t, h, w, radius, int(min_activity), A.ptr(motion), A.ptr(inliers),
                                       A.current_stream()), "pws_motion_fit")
    else:
        A.check(A.lib().pws_motion_fit_scaled(A.ptr(mv), A.ptr(sad), A.ptr(act), t, h, w, radius, int(min_activity), sx, sy, A.ptr(motion),
                                              A.ptr(inliers), A.current_stream()), "pws_motion_fit_scaled")
    return (motion, inliers, mv, sad, act) if return_blocks else (motion, inliers)


def _check_sigma(sigma, what, zero_ok=False):
    """``sigma`` as a float in (0, 256] (or [0, 256]); ValueError otherwise (NaN included)."""
    try:
        s = float(sigma)
    except (TypeError, ValueError):
        raise ValueError("%s: sigma must be a number of frames, got %r" % (what, sigma)) from None
    if not ((0.0 < s or (zero_ok and s == 0.0)) and s <= 256.0):
        raise ValueError("%s: sigma must lie in %s0, 256], got %r" % (what, "[" if zero_ok else "(", sigma))
    return s


def smooth_path(motion, sigma, scene_cuts=None):
    """The camera path a clip's per-pair motion adds up to, low-passed, and the per-frame corrections between the two (csrc/path_smooth.hip;
    include/pwstable.h pws_path_smooth has the definition): ``motion`` (T, 4) float64 on the device = (a, b, tx, ty) as ``global_motion``
    returns it -- row k maps a point of frame k to frame k-1; a NaN row counts as no motion -- and ``sigma``, the Gaussian's width in frames,
    in (0, 256].  Per scene (``scene_cuts``: sorted indices at which a new scene starts; the pair at a cut is not read, and every scene's
    path starts at zero) the pose of each frame in its scene's first frame, P = (log scale, angle, cx, cy), is accumulated, averaged over
    +-min(ceil(3 sigma), n-1) frames under the Gaussian with the path continued by odd reflection beyond the scene's ends (a steady pan is
    left alone at every frame), and D[k] = C_k^-1 o C^_k -- row-major 2 x 3 -- maps a position of the smoothed frame k to the measured
    frame's, in ``motion``'s pixels relative to the frame centre: what ``functional.compose_fields`` takes.  Returns (D (T, 6), path (T, 4)),
    float64 on the device, no synchronisation; one launch per scene, on slices.  Fixed order: the same bits on every run.
    ValueError: a tensor that is not (T, 4) float64 on the device, sigma outside (0, 256], bad cuts."""
    if not isinstance(motion, torch.Tensor) or not motion.is_cuda or motion.dtype != torch.float64 or motion.dim() != 2 or motion.shape[1] != 4:
        raise ValueError("smooth_path: motion must be a (T, 4) float64 tensor on the device")
    sigma = _check_sigma(sigma, "smooth_path")
    motion = motion.contiguous()
    T = motion.shape[0]
    cuts = _check_cuts(scene_cuts, T, "smooth_path") if scene_cuts is not None and len(scene_cuts) else []
    d = torch.empty((T, 6), device=motion.device, dtype=torch.float64)
    path = torch.empty((T, 4), device=motion.device, dtype=torch.float64)
    for a, b in (_scenes(T, cuts) if T else []):
        A.check(A.lib().pws_path_smooth(A.ptr(motion[a:b]), b - a, sigma, A.ptr(path[a:b]), A.ptr(d[a:b]), A.current_stream()), "pws_path_smooth")
    return d, path


def shutter_rates(motion, scene_cuts=None):
    """The camera's velocity at every frame of a clip, for the rolling-shutter correction (csrc/path_smooth.hip; include/pwstable.h
    pws_shutter_rates has the definition): ``motion`` (T, 4) float64 on the device as for ``smooth_path``.  Returns (T, 2, 4) float64 on
    the device: per frame k the rates (log scale, angle, x, y per frame interval) in frame k's own coordinates, [k, 0] from the pair ahead
    (motion[k+1]), [k, 1] from the pair behind (motion[k]) -- what ``functional.compose_fields(rates=)`` takes.  Per scene
    (``scene_cuts`` as for ``smooth_path``): rates never cross a cut, a scene's first and last frame use their one pair twice, a scene of
    one frame has zero rates; a NaN row counts as no motion.  No synchronisation; one launch per scene, on slices; the same bits on every run.
    ValueError: a tensor that is not (T, 4) float64 on the device, bad cuts."""
    if not isinstance(motion, torch.Tensor) or not motion.is_cuda or motion.dtype != torch.float64 or motion.dim() != 2 or motion.shape[1] != 4:
        raise ValueError("shutter_rates: motion must be a (T, 4) float64 tensor on the device")
    motion = motion.contiguous()
    T = motion.shape[0]
    cuts = _check_cuts(scene_cuts, T, "shutter_rates") if scene_cuts is not None and len(scene_cuts) else []
    rates = torch.empty((T, 2, 4), device=motion.device, dtype=torch.float64)
    for a, b in (_scenes(T, cuts) if T else []):
        A.check(A.lib().pws_shutter_rates(A.ptr(motion[a:b]), b - a, A.ptr(rates[a:b]), A.current_stream()), "pws_shutter_rates")
    return rates


def estimate_rolling_shutter(motion, mv, sad, activity, plane_hw, radius=16, min_activity=2000, pixel_scale=None, scene_cuts=None,
                             frame_height=None, return_terms=False):
    """The rolling-shutter share r of a clip, estimated from what ``global_motion(..., return_blocks=True)`` measured on it
    (csrc/shutter_estimate.hip; include/pwstable.h pws_shutter_terms / pws_shutter_estimate have the definition): ``motion`` (T, 4) float64
    and ``mv``, ``sad``, ``activity`` as that call returned them for (T, h, w) planes, ``plane_hw`` = (h, w), and the ``radius``,
    ``min_activity`` and ``pixel_scale`` that the call was given.  ``frame_height``: the frame's height in ``motion``'s pixels -- None: h
    times the scale's sy, which is h for the plane-pixel fit.  A rolling shutter leaves in the block vectors a displacement that no
    similarity absorbs: the block's share c of the readout (its row over the frame height, in [-1/2, 1/2]) times the change of the camera's
    velocity from the pair behind to this pair (``shutter_rates`` under ``scene_cuts``, computed here).  r is the least-squares coefficient
    of that regressor, over the blocks that the fit kept, of every pair with a real pair on both sides -- none within 2 frames of a cut or
    of the clip's ends, none next to a NaN row -- after the vectors and the regressor have each had their own similarity taken out.
    Returns a (4,) float64 device tensor (r_hat, se, D, n) [, terms (T, 4): per pair (sum e . z, sum z . z, sum e . e, blocks)], no
    synchronisation; one launch per scene and one for the estimate; fixed order, the same bits on every run.  D is the regressor's
    energy, n the blocks used; (NaN, inf, D, n) when D or the degrees of freedom are not positive (a still clip, T below 4).
    se is the formal least-squares standard error.  It tells a clip that holds information -- one with acceleration -- from one that
    does not (a tripod, a steady pan); it is NOT an error bar: the real errors are systematic (a first-order model, correlated sub-pixel
    bias) and measured several times larger on the analytic clips of tests/shutter_est_ref.py.  Not validated on real footage.
    ValueError: tensors other than these, on the device; shapes that do not fit (T, plane_hw, radius); a bad radius, pixel_scale,
    frame_height or cuts."""
    what = "estimate_rolling_shutter"
    if not isinstance(motion, torch.Tensor) or not motion.is_cuda or motion.dtype != torch.float64 or motion.dim() != 2 or motion.shape[1] != 4:
        raise ValueError("%s: motion must be a (T, 4) float64 tensor on the device" % what)
    try:
        h, w = (int(v) for v in plane_hw)
    except (TypeError, ValueError):
        raise ValueError("%s: plane_hw must be (h, w), got %r" % (what, plane_hw)) from None
    radius = int(radius)
    if not 1 <= radius <= 16:
        raise ValueError("%s: radius must be 1 .. 16, got %r" % (what, radius))
    if h - 2 * radius < 16 or w - 2 * radius < 16:
        raise ValueError("%s: a %d x %d plane holds no 16 x 16 block inside a margin of %d" % (what, h, w, radius))
    T = motion.shape[0]
    nby, nbx = (h - 2 * radius) // 16, (w - 2 * radius) // 16
    for name, x, dtype, shape in (("mv", mv, torch.int16, (T, nby, nbx, 2)), ("sad", sad, torch.int32, (T, nby, nbx, 5)),
                                  ("activity", activity, torch.int32, (T, nby, nbx))):
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != dtype or tuple(x.shape) != shape or not x.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s %s tensor on the device, as block_motion returns it for %d planes of %d x %d at "
                             "radius %d" % (what, name, shape, str(dtype).replace("torch.", ""), T, h, w, radius))
    sx, sy = (1.0, 1.0) if pixel_scale is None else _check_pixel_scale(pixel_scale, what)
    try:
        h0 = h * sy if frame_height is None else float(frame_height)
    except (TypeError, ValueError):
        raise ValueError("%s: frame_height must be None or a number of pixels, got %r" % (what, frame_height)) from None
    if not 1.0 < h0 <= 1e9:
        raise ValueError("%s: frame_height must lie in (1, 1e9], got %r" % (what, frame_height))
    motion = motion.contiguous()
    cuts = _check_cuts(scene_cuts, T, what) if scene_cuts is not None and len(scene_cuts) else []
    rates = shutter_rates(motion, scene_cuts=cuts or None)
    terms = torch.empty((T, 4), device=motion.device, dtype=torch.float64)
    for a, b in (_scenes(T, cuts) if T else []):
        A.check(A.lib().pws_shutter_terms(A.ptr(mv[a:b]), A.ptr(sad[a:b]), A.ptr(activity[a:b]), A.ptr(motion[a:b]), A.ptr(rates[a:b]), b - a, h, w,
                                          radius, int(min_activity), sx, sy, h0, A.ptr(terms[a:b]), A.current_stream()), "pws_shutter_terms")
    est = torch.empty((4,), device=motion.device, dtype=torch.float64)
    A.check(A.lib().pws_shutter_estimate(A.ptr(terms), T, A.ptr(est), A.current_stream()), "pws_shutter_estimate")
    return (est, terms) if return_terms else est


def _check_shutter(r, what):
    """``rolling_shutter`` as VideoStabilizer takes it: a float in [-1, 1] or "auto"; ValueError otherwise."""
    if isinstance(r, str):
        if r != "auto":
            raise ValueError("%s: rolling_shutter must be a number in [-1, 1] or \"auto\", got %r" % (what, r))
        return r
    return PF._check_rolling_shutter(r, what)


def _check_max_se(v, what):
    """``shutter_max_se`` as a float >= 0; ValueError otherwise (NaN included)."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s: shutter_max_se must be a number >= 0, got %r" % (what, v)) from None
    if not f >= 0.0:
        raise ValueError("%s: shutter_max_se must be a number >= 0, got %r" % (what, v))
    return f


def _check_limit(max_crop, levels, relax, sigma, what):
    """(max_crop or None, levels, relax) checked: max_crop in [0, 0.5] (NaN is a ValueError), levels an int in 1 .. 64, relax in (0, 1] --
    None: 1 / ceil(3 sigma), the strength recovers from 0 to 1 over the Gaussian's own reach (1.0 at sigma 0, where nothing is limited)."""
    if max_crop is not None:
        try:
            c = float(max_crop)
        except (TypeError, ValueError):
            raise ValueError("%s: max_crop must be None or a share of the frame in [0, 0.5], got %r" % (what, max_crop)) from None
        if not 0.0 <= c <= 0.5:   # (False for NaN)
            raise ValueError("%s: max_crop must lie in [0, 0.5], got %r" % (what, max_crop))
        max_crop = c
    try:
        lv = int(levels)
        if lv != levels:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("%s: limit_levels must be an integer in 1 .. 64, got %r" % (what, levels)) from None
    if not 1 <= lv <= 64:
        raise ValueError("%s: limit_levels must lie in 1 .. 64, got %r" % (what, levels))
    if relax is None:
        rx = 1.0 / max(1, int(math.ceil(3.0 * float(sigma))))
    else:
        try:
            rx = float(relax)
        except (TypeError, ValueError):
            raise ValueError("%s: limit_relax must be None or a number in (0, 1], got %r" % (what, relax)) from None
        if not 0.0 < rx <= 1.0:   # (False for NaN)
            raise ValueError("%s: limit_relax must lie in (0, 1], got %r" % (what, relax))
    return max_crop, lv, rx


def limit_rectangle(fraction, frame_hw, field_hw):
    """The nodes (i0, i1, j0, j1), inclusive, of every field cell that the centred window of ``fraction`` of the frame touches: with the
    window's (Ax, Bx, Ay, By) from ``functional.zoom_coefficients`` -- the float32 values that a later zoom to that window samples the field
    with -- j0 = floor(Ax), j1 = ceil(fmaf(Bx, fw - 1, Ax)), i0 and i1 alike, clamped to the lattice.  (The float64 sum Bx (fw-1) + Ax of
    float32 operands is exact at these magnitudes, so its one rounding to float32 is fmaf's.)"""
    import numpy as np
    h, w = int(frame_hw[0]), int(frame_hw[1])
    fh, fw = int(field_hw[0]), int(field_hw[1])
    win = PF._zoom_windows(_centred_window(float(fraction), h, w), 1, (h, w), "limit_path")
    ax, bx, ay, by = (float(v) for v in PF.zoom_coefficients(win, (h, w), (fh, fw))[0].tolist())

    def span(a, b, n):
        lo = int(math.floor(a))
        hi = int(math.ceil(float(np.float32(b * (n - 1) + a))))
        return min(max(lo, 0), n - 1), min(max(hi, 0), n - 1)
    i0, i1 = span(ay, by, fh)
    j0, j1 = span(ax, bx, fw)
    return i0, i1, j0, j1


def limit_path(d, fields, frame_hw, fraction, levels=16, relax=1.0, scene_cuts=None, rates=None, rolling_shutter=0.0, align_corners=False,
               mode="bilinear"):
    """Crop-bounded smoothing, the step on its own (csrc/path_limit.hip, csrc/field_reach.hip; include/pwstable.h pws_path_levels,
    pws_field_reach and pws_path_limit have the definitions): per frame, as much of the smoothing correction as keeps a window of the
    output covered by the source, eased over time.  ``d`` (T, 6) float64 on the device as ``smooth_path`` returns it (similarities);
    ``fields`` (T, fh, fw, 2) float32 on the device, the fields that ``functional.compose_fields`` will fold d into, read in place;
    ``fraction`` = k in (0, 1]: the protected window is the centred window of that fraction of the ``frame_hw`` = (H0, W0) frame
    (``_centred_window``: the one ``run_video(zoom=k)`` shows).
    D_t(lam) is the correction scaled back along (log scale, angle, translation): exp(lam ls) Rot(lam phi), lam (d2, d5).  For lam = l /
    levels, l = 0 .. levels, ``pws_field_reach`` counts the nodes of ``limit_rectangle`` -- every node of every field cell the window
    touches -- whose composed value would sample outside the source (``compose_fields``' own node function and ``zoom_fields``' coverage
    rule with ``align_corners`` and ``mode``; with ``rates`` and ``rolling_shutter`` the row-dependent composition).  need[t] is the
    largest level up to which every count is zero (-1: the field alone leaves the window uncovered), the raw strength max(need, 0) /
    levels; inside each scene (``scene_cuts`` as for ``smooth_path``) the strength is the largest sequence below it that changes by at
    most ``relax`` per frame (``zoom_schedule``'s two sweeps; never across a cut); d_limited[t] is d[t] verbatim at strength 1, else
    D_t(strength[t]).  The source rectangle is convex and the warps interpolate the field linearly between nodes, so zero uncovered
    nodes in the rectangle means that zoom=k shows no wedge.  After the sweeps a strength lies between grid levels, where feasibility is
    not proven: the last value returned counts the rectangle's uncovered nodes under d_limited itself.
    Returns (d_limited (T, 6) float64, strength (T,) float64, need (T,) int32, counts (T,) int32), on the device, no synchronisation;
    3 + (number of scenes) launches and two small clears.  Integer counts and one fixed order: the same bits on every run.
    ValueError: tensors other than these, fraction outside (0, 1], levels outside 1 .. 64, relax outside (0, 1], rolling_shutter outside
    [-1, 1], an unknown mode, bad cuts, a frame below 2 x 2 pixels."""
    if mode not in PF.INTERPOLATIONS:
        raise ValueError("mode must be one of %s, got %r" % (PF.INTERPOLATIONS, mode))
    r = PF._check_rolling_shutter(rolling_shutter, "limit_path")
    rows = r != 0.0 and rates is not None
    for name, t, dtype in (("d", d, torch.float64), ("fields", fields, torch.float32)) + ((("rates", rates, torch.float64),) if rows else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
            raise ValueError("limit_path: %s must be a %s tensor on the device" % (name, dtype))
    if fields.dim() != 4 or fields.shape[3] != 2 or fields.shape[1] < 2 or fields.shape[2] < 2:
        raise ValueError("limit_path: fields must be (T, fh, fw, 2) with fh, fw >= 2, got %s" % (tuple(fields.shape),))
    T, fh, fw = fields.shape[:3]
    if tuple(d.shape) != (T, 6):
        raise ValueError("limit_path: d must be (%d, 6), got %s" % (T, tuple(d.shape)))
    if rows and tuple(rates.shape) != (T, 2, 4):
        raise ValueError("limit_path: rates must be (%d, 2, 4), got %s" % (T, tuple(rates.shape)))
    h0, w0 = int(frame_hw[0]), int(frame_hw[1])
    if h0 < 2 or w0 < 2:
        raise ValueError("limit_path: the frame must be at least 2 x 2 pixels, got %d x %d" % (w0, h0))
    try:
        k = float(fraction)
    except (TypeError, ValueError):
        raise ValueError("limit_path: fraction must be a number in (0, 1], got %r" % (fraction,)) from None
    if not 0.0 < k <= 1.0:
        raise ValueError("limit_path: fraction must lie in (0, 1], got %r" % (fraction,))
    _, levels, relax = _check_limit(None, levels, relax, 0.0, "limit_path")
    cuts = _check_cuts(scene_cuts, T, "limit_path") if scene_cuts is not None and len(scene_cuts) else []
    d, fields = d.contiguous(), fields.contiguous()
    rates = rates.contiguous() if rows else None
    dev = d.device
    d_out = torch.empty((T, 6), device=dev, dtype=torch.float64)
    strength = torch.empty((T,), device=dev, dtype=torch.float64)
    need = torch.empty((T,), device=dev, dtype=torch.int32)
    left = torch.empty((T, 1), device=dev, dtype=torch.int32)
    if T == 0:
        return d_out, strength, need, left.reshape(0)
    i0, i1, j0, j1 = limit_rectangle(k, (h0, w0), (fh, fw))
    L, stream = A.lib(), A.current_stream()
    table = torch.empty((T, levels + 1, 6), device=dev, dtype=torch.float64)
    counts = torch.empty((T, levels + 1), device=dev, dtype=torch.int32)

    def reach(tab, lv, out):
        A.check(L.pws_field_reach(A.ptr(fields), T, fh, fw, A.ptr(tab), lv, A.ptr(rates), r if rows else 0.0, i0, i1, j0, j1, h0, w0,
                                  PF._ac(align_corners), int(mode == "bicubic"), A.ptr(out), stream), "pws_field_reach")
    A.check(L.pws_path_levels(A.ptr(d), T, levels, A.ptr(table), stream), "pws_path_levels")
    reach(table, levels, counts)
    for a, b in _scenes(T, cuts):
        A.check(L.pws_path_limit(A.ptr(d[a:b]), A.ptr(counts[a:b]), b - a, levels, relax, A.ptr(need[a:b]), A.ptr(strength[a:b]),
                                 A.ptr(d_out[a:b]), stream), "pws_path_limit")
    reach(d_out, 0, left)   # (T, 6) is a (T, 1, 6) table
    return d_out, strength, need, left.reshape(T)


def _signal_score(v):
    """One signal's stability score over a scene of m frames; v[k] is the motion of pair k (v[0] is not read)."""
    import numpy as np
    m = len(v)
    p = np.zeros(m, np.float64)
    for k in range(1, m):
        p[k] = p[k - 1] + v[k]
    p = p - (p[0] + (p[m - 1] - p[0]) * (np.arange(m, dtype=np.float64) / float(m - 1)))
    e = np.abs(np.fft.fft(p)) ** 2
    e = e[1:m // 2]
    total = float(e.sum())
    return 1.0 if total == 0.0 else float(e[:5].sum()) / total


def stability_scores(motion, scene_cuts=None):
    """The PWStableNet paper's stability metric over a clip's per-pair motion (``global_motion``; (T, 4) = (a, b, tx, ty), a tensor on either
    side or an array; host arithmetic, float64).  Per scene -- ``scene_cuts``: sorted indices at which a new scene starts; the pair at a cut
    does not count -- three signals are scored, tx, ty and theta = atan2(b, a): the path p[0] = 0, p[k] = p[k-1] + v[k] over the scene's m
    frames, minus the straight line through its two end points; E = |FFT(p)|^2 over bins 1 .. m//2 - 1; the score is the first five bins
    over all of them (1.0 when the total is 0: a still camera).  The published definition takes the FFT of the raw path, under which a steady
    pan's own ramp hides the shake (INTEGRATION.md has the figures); the line is the one deviation.  A scene of fewer than 24 frames, or with
    a NaN pair, scores NaN.  Returns {"stability", "translation", "rotation": the clip's values -- the frame-weighted mean of the scored
    scenes, NaN without any -- and "scenes": [{"start", "end", "translation" = min(score x, score y), "rotation", "stability" = the smaller
    of the two}]}.  The scores are pinned on synthetic clips only; no real footage or trained weights were available to validate them."""
    import numpy as np
    if isinstance(motion, torch.Tensor):
        motion = motion.detach().to("cpu", torch.float64).numpy()
    motion = np.asarray(motion, np.float64)
    if motion.ndim != 2 or motion.shape[1] != 4:
        raise ValueError("stability_scores: motion must be (T, 4): a, b, tx, ty")
    T = motion.shape[0]
    cuts = _check_cuts(scene_cuts, T, "stability_scores") if scene_cuts is not None and len(scene_cuts) else []
    nan, scenes = float("nan"), []
    for a, b in _scenes(T, cuts):
        rows = motion[a:b]
        if b - a < 24 or not np.isfinite(rows[1:]).all():
            tr = ro = nan
        else:
            tr = min(_signal_score(rows[:, 2]), _signal_score(rows[:, 3]))
            ro = _signal_score(np.arctan2(rows[:, 1], rows[:, 0]))
        scenes.append({"start": a, "end": b, "translation": tr, "rotation": ro, "stability": min(tr, ro) if tr == tr else nan})

    def clip(key):
        ok = [s for s in scenes if s[key] == s[key]]
        return sum(s[key] * (s["end"] - s["start"]) for s in ok) / sum(s["end"] - s["start"] for s in ok) if ok else nan
    return {"stability": clip("stability"), "translation": clip("translation"), "rotation": clip("rotation"), "scenes": scenes}


def find_scene_cuts(scores, threshold=0.25, min_scene=16):
    """The cut rule over a clip's ``scene_scores`` (a tensor on either side, an array or a sequence; host arithmetic): the sorted indices t,
    1 <= t < T, at which a new scene starts.  t is a cut if ``score[t] > threshold`` and t lies at least ``min_scene`` frames after the
    previous accepted cut (or after frame 0); a candidate closer than that is dropped and does not restart the count (a photo flash gives two
    high scores a frame or two apart, and one cut at most).  The rule is causal -- nothing after t is read -- so run_video can apply it
    chunk by chunk while the clip is still uploading."""
    if isinstance(scores, torch.Tensor):
        scores = scores.detach().to("cpu", torch.float32).tolist()
    cuts, last = [], 0
    for t, v in enumerate(scores):
        if t >= 1 and float(v) > threshold and t - last >= min_scene:
            cuts.append(t)
            last = t
    return cuts


def _check_cuts(cuts, n, what):
    """scene_cuts as a list of ints: sorted, unique, within 1 .. n-1 (ValueError otherwise)."""
    if isinstance(cuts, torch.Tensor):
        cuts = cuts.tolist()
    try:
        cuts = [int(c) for c in cuts]
    except (TypeError, ValueError):
        raise ValueError("%s: scene_cuts must be a sequence of frame indices" % what) from None
    if any(not 1 <= c < n for c in cuts) or any(c2 <= c1 for c1, c2 in zip(cuts, cuts[1:])):
        raise ValueError("%s: scene_cuts must be sorted, unique and within 1 .. %d, got %r" % (what, n - 1, cuts))
    return cuts


def _scenes(n, cuts):
    """The scenes [a, b) that the cuts split 0 .. n into."""
    edges = [0] + list(cuts) + [n]
    return list(zip(edges[:-1], edges[1:]))


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
    scenes = _scenes(T, _check_cuts(scene_cuts, T, "auto_crop_window")) if scene_cuts is not None and len(scene_cuts) else [(0, T)]
    for i in (i for a, b in scenes for i in range(a + half + 1, b - half)):
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
    for a, b in (_scenes(T, _check_cuts(scene_cuts, T, "zoom_schedule")) if scene_cuts is not None and len(scene_cuts) else [(0, T)]):
        for t in range(a + 1, b):
            k[t] = min(k[t], k[t - 1] + speed)
        for t in range(b - 2, a - 1, -1):
            k[t] = min(k[t], k[t + 1] + speed)
    return [_centred_window(v, h0, w0) for v in k]


def _windows(gray_padded, start, count, period):
    """(count, period+1, 256, 256) windows: window b covers padded frames [start+b, start+b+period].  An OVERLAPPING VIEW of the
    plane buffer (sample stride = one plane): the generator's first layer reads it in place (pws_netg_opts.x_sample_stride); no
    31-plane copy per window (65 MB per batch of 8)."""
    h, w = gray_padded.shape[-2:]
    return torch.as_strided(gray_padded, (count, period + 1, h, w), (h * w, h * w, w, 1),
                            storage_offset=gray_padded.storage_offset() + start * h * w)


class VideoStabilizer:
    def __init__(self, netG, batch=32, period=30, device=None, swap_rb=False, interpolation="bilinear", borders="black", rigidity=0.0,
                 mosaic_radius=8, edge="pad", metrics=False, smooth=0.0, rolling_shutter=0.0, wobble=0.0, max_crop=None, limit_levels=16,
                 limit_relax=None, shutter_max_se=0.02):
        self.net = netG
        # run_video low-passes the NON-RIGID part of the clip's fields along time: each field minus its fitted homography, under a Gaussian of
        # `wobble` frames, in (0, 5] (functional.wobble_fields).  The generator regresses every field from that frame's own window, and the
        # local part of consecutive fields shimmers; rigidity removes that part altogether, this keeps it and steadies it.  0: no launch, no
        # allocation, every path as it was
        self.wobble = PF._check_wobble(wobble, "VideoStabilizer", zero_ok=True)
        self.wobble_removed = None   # wobble > 0, of the last run_video, on the device: (T,) float32, per frame the largest distance in source
        self.wobble_unfit = None     # pixels by which the filter moved a node; (T,) int32, the nodes that kept their value (not usable)
        # run_video folds the shake that the fields LEAVE in the clip back into them: the global motion of the planes as the kept fields warp
        # them is measured, the camera path low-passed with a Gaussian of `smooth` frames (smooth_path) and every frame's correction composed
        # into its field (functional.compose_fields) before the one warp.  0: no launch, no allocation, every path as it was
        self.smooth = _check_sigma(smooth, "VideoStabilizer", zero_ok=True)
        self.smooth_motion = self.smooth_inliers = None       # smooth > 0, of the last run_video, on the device: (T, 4) float64 / (T,) int32, the
        self.smooth_path = self.smooth_correction = None      # motion the fields left (frame pixels); (T, 4) its path, (T, 6) the corrections D;
        self.smooth_uncovered = None                          # (T,) int32, the composed fields' nodes that sample outside the source
        # the share of the frame interval that the sensor's readout takes from the top row to the bottom row, in [-1, 1] (negative: bottom to
        # top); a property of the camera, which the user supplies.  Not 0: the correction that smoothing composes into each field depends on
        # the row (shutter_rates, functional.compose_fields(rates=, rolling_shutter=)), so that the skew and wobble of a CMOS readout under
        # shake come out with the shake.  It needs the motion that smoothing measures and the second pass that smoothing owns
        # "auto": run_video estimates it from the block vectors that smoothing measures (estimate_rolling_shutter) and uses the estimate,
        # clamped to [-1, 1], when it is finite and its formal standard error is at most shutter_max_se; otherwise 0.0, no correction.  The
        # standard error is a gate against clips without information (a tripod, a steady pan), not an error bar; 0.02 is a judgement that
        # no footage here can fit, like zoom_speed: the analytic clips of tests/shutter_est_ref.py measure 0.005 .. 0.010 where the estimate
        # is good to 0.07, and 0.78 on a steady pan
        self.rolling_shutter = _check_shutter(rolling_shutter, "VideoStabilizer")
        self.shutter_max_se = _check_max_se(shutter_max_se, "VideoStabilizer")
        self.shutter_estimate = None        # rolling_shutter="auto", of the last run_video: (4,) float64 on the device = (r_hat, se, D, blocks),
        self.rolling_shutter_used = None    # and the r that the gate let through, a float
        if self.rolling_shutter != 0.0 and self.smooth == 0.0:
            raise ValueError("VideoStabilizer: rolling_shutter=%r needs smooth > 0 (the correction uses the motion that smoothing measures and "
                             "its second pass)" % (rolling_shutter,))
        self.shutter_rates = None   # rolling_shutter != 0, of the last run_video, on the device: (T, 2, 4) float64, shutter_rates' rows
        # the crop budget of smoothing: the share of the frame, per axis, that the viewer is prepared to lose, in [0, 0.5].  Each frame takes
        # as much of its correction as keeps the centred window of the fraction 1 - max_crop covered by the source (limit_path: the share is
        # searched on limit_levels + 1 grid levels, on the fields themselves) and the share changes by at most limit_relax per frame.
        # limit_relax=None: 1 / ceil(3 smooth), the strength recovers from 0 to 1 over the Gaussian's own reach -- a judgement that no
        # footage here can fit, like zoom_speed.  None: no launch, no allocation, every path as it was
        self.max_crop, self.limit_levels, relax = _check_limit(max_crop, limit_levels, limit_relax, self.smooth, "VideoStabilizer")
        self.limit_relax = None if limit_relax is None else relax   # (None is resolved against the call's smooth in run_video)
        if self.max_crop is not None and self.smooth == 0.0:
            raise ValueError("VideoStabilizer: max_crop=%r needs smooth > 0 (it bounds the correction that smoothing composes)" % (max_crop,))
        self.limit_strength = self.limit_need = None          # max_crop, of the last run_video, on the device: (T,) float64 in [0, 1]; (T,) int32, the
        self.limit_uncovered = None                           # raw level (-1: the field alone leaves the window uncovered); (T,) int32, the window's
        self.smooth_correction_unlimited = None               # nodes still outside under the D that was composed; (T, 6), what smooth_path returned
        # run_video measures the clip it stabilises: the global motion of the input and of the output planes (global_motion), and from it
        # and the per-frame homographies the paper's three metrics (stability_report).  False: no launch, no allocation, every path as it was
        self.metrics = bool(metrics)
        self.motion_in = self.motion_out = None                    # metrics: (T, 4) float64 = (a, b, tx, ty) per pair of the last run_video's
        self.motion_inliers_in = self.motion_inliers_out = None    # input / output planes and (T,) int32 inlier counts, on the device
        self._report = None
        # how far run / run_video pull each frame's field towards the homography fitted to it (functional.rigid_fields): 0 = the field as the
        # generator regressed it (no fit, no launch), 1 = every frame warped by its homography alone -- no local distortion, and no parallax
        # correction either
        self.rigidity = PF._check_rigidity(rigidity, "VideoStabilizer")
        if borders not in PF.BORDERS:
            raise ValueError("borders must be one of %s, got %r" % (PF.BORDERS, borders))
        # what run / run_video show where a frame's field samples outside the source: the warp's pad colour, or -- "keep", vid.stab's
        # crop=keep -- the previous output frame of the scene (functional.keep_borders_, one more launch per batch and scene)
        # "mosaic": the temporally nearest stabilised frame of the scene that covers the pixel, at most mosaic_radius frames into the past or
        # the future (functional.mosaic_borders_, one launch per scene piece once the neighbours are warped).  8 is a judgement -- about a
        # quarter second at 30 fps -- that no footage here can fit.
        self.borders = borders
        # how the SOURCE continues beyond its rim where a wedge still shows it ("black", and what "mosaic" finds no donor for): "pad" -- the
        # warp's blend with the pad colour, every path as it was -- or "clamp" / "mirror": functional.edge_borders_ right after each warp,
        # from the batch's own source frames and the field that warped them (one more launch per batch; no other frame is read)
        if edge not in PF.EDGES:
            raise ValueError("edge must be one of %s, got %r" % (PF.EDGES, edge))
        if edge != "pad" and borders == "keep":
            raise ValueError("edge=%r has nothing to fill with borders=\"keep\", which never shows the pad colour: choose one" % (edge,))
        self.edge = edge
        self.mosaic_radius = int(mosaic_radius)
        if not 1 <= self.mosaic_radius <= PF.MOSAIC_MAX_RADIUS:
            raise ValueError("mosaic_radius must be 1 .. %d (the kernel keeps one window bit per frame), got %r" % (PF.MOSAIC_MAX_RADIUS, mosaic_radius))
        self.mosaic_unfilled = None   # borders="mosaic": per frame of the last run / run_video, the Y (BGR: pixel) positions no frame within the
        #                               radius covers: (T,) int32 on the device; None for the other border modes
        if interpolation not in PF.INTERPOLATIONS:
            raise ValueError("interpolation must be one of %s, got %r" % (PF.INTERPOLATIONS, interpolation))
        self.interpolation = interpolation   # how run / run_video make an output pixel: 4 taps, or grid_sample(mode="bicubic")'s 16
        self.swap_rb = bool(swap_rb)   # uint8 frames only: BGR (cv2) in, RGB out, as main_new.py:679
        self.batch = int(batch)
        self.period = int(period)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        # grid_sample follows the generator's coordinate convention (UnetGenerator.align_corners: torch >= 1.3 default False;
        # True for checkpoints trained under the reference's pinned torch 0.4)
        self.align_corners = bool(getattr(getattr(netG, "module", netG), "align_corners", False))
        self._lanes = []   # compute streams of run_video(in_flight > 1)
        self.scene_cuts = []   # the cuts the last run_video used (frames' index space)
        self.scene_wait_s = 0.0   # host time the last run_video(scene_cuts="auto") spent waiting for scores
        self.zoom_windows = None     # the T windows the last run / run_video with a zoom used (None without one)
        self.zoom_uncovered = None   # and, per frame, the zoomed field's nodes that sample outside the source: (T,) int32 on the device
        self.rigid_residual = None   # rigidity > 0: per frame of the last run / run_video, how far the generator's field was from its fitted
        self.rigid_unfit = None      # homography (source pixels, (T,) float32) and the nodes no homography applied to ((T,) int32); on the device

    def _pad(self, gray, halo_left, halo_right):
        """Replicates the first / last available frame so that every frame owns a full window (reference :627-633)."""
        half = self.period // 2
        need_l, need_r = half - halo_left, half - halo_right
        parts = []
        if need_l > 0:
            parts.append(gray[:1].expand(need_l, -1, -1))
        parts.append(gray)
        if need_r > 0:
            parts.append(gray[-1:].expand(need_r, -1, -1))
        return torch.cat(parts, 0) if len(parts) > 1 else gray

    def _layout(self, gray, halo_left, halo_right, T, scene_cuts=None):
        """The padded plane buffer and the generator batches of run(): [(s, e, start)] -- frames s .. e-1 (output positions) form one call
        whose windows begin at padded plane start, start + 1, ...
        With scene cuts (indices into ``gray``, halos included) plane j of the window of gray frame g in scene [a, b) is
        gray[clamp(g - half + j, a, b - 1)]: the buffer holds, scene after scene, [first frame x need_l, scene, last frame x need_r] (a
        frame's window starts 2 * half planes further on for each earlier scene), and the batches restart at every scene's first frame,
        because a strided view cannot span a cut: a scene sees the generator calls that a clip made of it alone would see.  Scenes that lie
        wholly inside a halo hold no frame to stabilise and are left out."""
        if not scene_cuts:
            gp = self._pad(gray, halo_left, halo_right).contiguous()
            return gp, [(s, min(T, s + self.batch), s) for s in range(0, T, self.batch)]
        half, n = self.period // 2, gray.shape[0]
        parts, batches, pos = [], [], 0
        for a, b in _scenes(n, scene_cuts):
            ca, cb = max(a, halo_left), min(b, halo_left + T)   # the scene's frames to stabilise
            if ca >= cb:
                continue
            need_l = half if a > 0 else max(0, half - halo_left)
            need_r = half if b < n else max(0, half - halo_right)
            if need_l:
                parts.append(gray[a:a + 1].expand(need_l, -1, -1))
            parts.append(gray[a:b])
            if need_r:
                parts.append(gray[b - 1:b].expand(need_r, -1, -1))
            first = pos + need_l - half - a   # the window of gray frame g starts at padded plane first + g
            for s in range(ca, cb, self.batch):
                batches.append((s - halo_left, min(cb, s + self.batch) - halo_left, first + s))
            pos += need_l + (b - a) + need_r
        return torch.cat(parts, 0), batches

    def _fields(self, gray, halo_left, halo_right, out, scene_cuts=None):
        """The generator half of run(): the fields of the out.shape[0] frames into ``out`` (T, 256, 256, 2), in the batches run()
        forms (the same windows per generator call: the same fields bit for bit).  The copy also frees a graph's static output."""
        gp, batches = self._layout(gray.contiguous(), halo_left, halo_right, out.shape[0], scene_cuts)
        for s, e, start in batches:
            out[s:e].copy_(self.net(_windows(gp, start, e - s, self.period), False))

    @torch.no_grad()
    def run(self, gray, frames, halo_left=0, halo_right=0, out=None, pixel_format="bgr24", scene_cuts=None, keep_from=None, _keep_wait=None,
            zoom=None, _zoom_unc=None, _rigid_stats=None, _mosaic_pad=None, _hom_out=None):
        """gray: (T + halo_left + halo_right, 256, 256) float32 in [-1,1] (``x/255*2-1`` as the reference, :650) for the T
        frames to stabilise plus whatever real neighbours exist on either side (up to period//2); frames: (T, C, H, W)
        float32 0..255, or (T, H, W, 3) uint8 as OpenCV delivers them (then the warp runs in the uint8 kernel: 4x less
        PCIe and HBM traffic per frame, ``self.swap_rb`` applies the reference's BGR->RGB).  Tensors may be on the device or in
        (pinned) host memory.  Returns a tensor of the frames' shape and dtype on the inputs' side.  Every warp below runs with
        ``self.interpolation`` ("bilinear", or "bicubic": functional.upsample_grid_sample*(mode="bicubic")); nothing else depends on it.
        pixel_format = "nv12" / "i420": frames are packed 4:2:0 (T, H * 3 // 2, W) uint8 (H even, W % 4 == 0), warped plane by plane in
        the fused YUV kernel (functional.upsample_grid_sample_yuv420: BT.601 black padding); ``self.swap_rb`` does not apply.
        pixel_format = "p010" / "i010": the same for 10-bit frames (T, H * 3 // 2, W) uint16 (functional.upsample_grid_sample_yuv420_16).
        pixel_format = "nv16" / "i422" / "p210" / "i210" (4:2:2, (T, 2 * H, W)) and "i444" / "i410" (4:4:4, (T, 3 * H, W)): the same, plane by
        plane with the chroma planes at their own size (functional.upsample_grid_sample_yuv).
        scene_cuts: sorted indices into ``gray`` (halo frames count; 1 .. len - 1) at which a new scene starts.  Windows end at them as they
        end at the clip's ends -- the scene's first / last frame is repeated (_layout) -- and the batches restart at every scene, so a scene
        is stabilised exactly as the clip of that scene alone would be.  None or empty: one scene.
        borders="keep" (integer frames only; float frames are a ValueError): after each batch's warp ``functional.keep_borders_`` runs over
        it -- a batch never spans a cut, so it is one segment -- starting from the previous batch's last OUTPUT frame, or, at a scene's first
        frame, from that frame's own SOURCE.  keep_from: the output frame (device tensor, one frame of the frames' layout, before any resize)
        that precedes frames[0] in its scene, for a clip processed in several calls (run_video passes each chunk's last frame on); without
        it frames[0] starts from its source -- so a shard with halo_left > 0 has no history and does not promise the unsharded clip's
        bytes in its wedges.
        zoom: one window (x0, x1, y0, y1) or (T, 4) windows for the T frames, in source-pixel edge coordinates (functional.zoom_fields): each
        batch's field goes through ``zoom_fields`` after the generator and before the warp, so the output shows that window of the stabilised
        frame at the full frame size, still resampled once.  The windows are left in ``self.zoom_windows``, the per-frame counts of field
        nodes that sample outside the source in ``self.zoom_uncovered``.  Not with borders="keep" (ValueError).
        borders="mosaic" (integer frames only; float frames are a ValueError): the call's own frames are the only donors.  Every batch is
        warped with black borders into one device buffer, the fields that warped them (after rigidity) are kept beside it, and once every
        batch is warped ``functional.mosaic_borders_`` runs once per scene piece (slices along dim 0, cut at ``scene_cuts``) with
        ``self.mosaic_radius``; then the frames are copied out.  Halo frames are never warped and so are no donors: a shard's first and last
        ``mosaic_radius`` frames do not promise the unsharded clip's bytes inside the wedges.  ``self.mosaic_unfilled`` (T,) int32 is left on
        the device (no synchronisation).  Not with a zoom (ValueError).  (_mosaic_pad, run_video's: the buffers get that many spare frames at
        either end and are returned unfilled, (warped, fields), instead of the output.)
        VideoStabilizer(rigidity=r), r > 0: each batch's field is fitted (``field_homography``) and blended towards its homography
        (``functional.rigid_fields``, into a fresh tensor: the generator's output may be a graph's static buffer) right after the generator;
        the zoom, the warp and borders="keep" all see the adjusted field.  Nothing here depends on other frames, so halos are fine; frames
        below the fit's 600 x 300 lattice are a ValueError.  ``self.rigid_residual`` (T,) float32 and ``self.rigid_unfit`` (T,) int32 are left on
        the device (None at rigidity 0, which takes no new path).
        VideoStabilizer(edge="clamp" | "mirror") (integer frames only; float frames are a ValueError): right after each batch's warp
        ``functional.edge_borders_`` samples every uncovered pixel again from the batch's own source frames, continued beyond their rim, with
        the field that warped (after rigidity and zoom); with borders="mosaic" on the batch's slice of the buffer, before the mosaic pass,
        so donors still win and the unfilled positions show the edge fill.  Nothing crosses a frame: halos, cuts and shards change nothing.
        VideoStabilizer(smooth=sigma) does nothing here: run() does not smooth.  The path needs every field of the scene before the first
        warp, which is run_video's two-pass route."""
        half = self.period // 2
        keep = self.borders == "keep"
        rigid = self.rigidity > 0.0
        mosaic = self.borders == "mosaic"
        if zoom is not None and keep:
            raise ValueError("run: zoom removes the wedges that borders=\"keep\" fills: choose one")
        if zoom is not None and mosaic:
            raise ValueError("run: zoom removes the wedges that borders=\"mosaic\" fills: choose one")
        if mosaic and frames.dtype not in (torch.uint8, torch.uint16):
            raise ValueError("run: borders=\"mosaic\" is for the integer pixel formats (uint8 / uint16 frames), got %s" % (frames.dtype,))
        if _mosaic_pad is None:
            self.mosaic_unfilled = torch.empty((frames.shape[0],), device=self.device, dtype=torch.int32) if mosaic else None
        if keep and frames.dtype not in (torch.uint8, torch.uint16):
            raise ValueError("run: borders=\"keep\" is for the integer pixel formats (uint8 / uint16 frames), got %s" % (frames.dtype,))
        edging = self.edge != "pad"
        if edging and frames.dtype not in (torch.uint8, torch.uint16):
            raise ValueError("run: edge=%r is for the integer pixel formats (uint8 / uint16 frames), got %s" % (self.edge, frames.dtype))
        fmt = PF.frame_format(pixel_format, frames, "run", float_frames=True)   # (from here on the format is this record)
        if not (0 <= halo_left <= half and 0 <= halo_right <= half):
            raise ValueError("halo must be within [0, %d]" % half)
        T = frames.shape[0]
        if gray.shape[0] != T + halo_left + halo_right:
            raise ValueError("gray has %d frames, expected %d + %d + %d" % (gray.shape[0], T, halo_left, halo_right))
        on_host = not frames.is_cuda
        dev = self.device
        cuts = _check_cuts(scene_cuts, gray.shape[0], "run") if scene_cuts is not None else None
        gray_d = gray.to(dev, non_blocking=True) if not gray.is_cuda else gray  # 256 KB per frame: copied once
        if out is None:
            out = torch.empty_like(frames, pin_memory=on_host) if on_host else torch.empty_like(frames)
        if zoom is not None or rigid or _hom_out is not None:
            frame_hw = fmt.frame_shape(frames)[1:]
        if rigid:
            _check_lattice(int(frame_hw[0]), int(frame_hw[1]), "rigidity > 0")
        if _rigid_stats is not None:   # run_video's, a slice per chunk: it publishes the whole tensors itself, once every chunk is issued
            rres, runf = _rigid_stats
        else:
            rres, runf = (torch.empty((T,), device=dev, dtype=torch.float32), torch.empty((T,), device=dev, dtype=torch.int32)) if rigid else (None, None)
            self.rigid_residual, self.rigid_unfit = rres, runf
        if zoom is not None:
            self.zoom_windows = PF._zoom_windows(zoom, T, frame_hw, "run")
            self.zoom_uncovered = _zoom_unc if _zoom_unc is not None else torch.empty((T,), device=dev, dtype=torch.int32)
            zcoef = None   # (the field's size is the generator's to say: formed at the first batch, uploaded once)
        if T == 0:
            return out
        gp, batches = self._layout(gray_d.contiguous(), halo_left, halo_right, T, cuts)
        compute = torch.cuda.current_stream(dev)
        h2d, d2h = (torch.cuda.Stream(dev), torch.cuda.Stream(dev)) if on_host else (None, None)

        def fetch(k):
            return _prefetch(frames, batches[k][0], batches[k][1], h2d, dev)
        nxt = fetch(0)
        pending = []
        cutset, prev = set(cuts or ()), None
        pad, wall, fall = _mosaic_pad or 0, None, None   # borders="mosaic": the call's warped frames and fields, `pad` spare frames at either end
        for k, (s, e, start) in enumerate(batches):
            cur, ev = nxt
            if k + 1 < len(batches):
                nxt = fetch(k + 1)  # overlaps with this batch's compute
            if ev is not None:
                compute.wait_event(ev)
            win = _windows(gp, start, e - s, self.period)
            field = self.net(win, False)
            if _hom_out is not None:   # run_video(metrics=True): the raw field's fit is kept, (T, 9) and (T, 4) slices of this call's frames
                field = field.contiguous()
                hom = _hom_out[0][s:e]
                _field_homography(field, int(frame_hw[0]), int(frame_hw[1]), hom, _hom_out[1][s:e])
                if rigid:
                    field = PF._field_rigid(field, hom, frame_hw, self.rigidity, torch.empty_like(field), rres[s:e], runf[s:e])
            elif rigid:
                field = field.contiguous()
                hom = torch.empty((e - s, 9), device=dev, dtype=torch.float64)
                _field_homography(field, int(frame_hw[0]), int(frame_hw[1]), hom, torch.empty((e - s, 4), device=dev, dtype=torch.float32))
                field = PF._field_rigid(field, hom, frame_hw, self.rigidity, torch.empty_like(field), rres[s:e], runf[s:e])
            if zoom is not None:
                if zcoef is None:
                    zcoef = PF.zoom_coefficients(self.zoom_windows, frame_hw, field.shape[1:3]).to(dev, non_blocking=True)
                field = field.contiguous()
                field = PF._field_zoom(field, zcoef[s:e], frame_hw, self.align_corners, self.interpolation, torch.empty_like(field),
                                       self.zoom_uncovered[s:e])
            if mosaic:   # black borders into the call's buffer; the fill needs every batch
                if wall is None:
                    wall = torch.empty((T + 2 * pad,) + tuple(frames.shape[1:]), device=dev, dtype=frames.dtype)
                    fall = torch.empty((T + 2 * pad,) + tuple(field.shape[1:]), device=dev, dtype=torch.float32)
                PF.warp(cur.contiguous(), field, fmt, swap_rb=self.swap_rb, align_corners=self.align_corners, out=wall[pad + s:pad + e],
                        mode=self.interpolation)
                if edging:   # before the mosaic pass: donors are read only where they are covered, so exactly the unfilled positions show it
                    PF.edge_borders_(wall[pad + s:pad + e], cur.contiguous(), field, self.edge, pixel_format, swap_rb=self.swap_rb,
                                     align_corners=self.align_corners, mode=self.interpolation)
                fall[pad + s:pad + e].copy_(field)
                if on_host:
                    cur.record_stream(compute)
                continue
            warped = PF.warp(cur.contiguous(), field, fmt, swap_rb=self.swap_rb, align_corners=self.align_corners, mode=self.interpolation)
            if edging:
                PF.edge_borders_(warped, cur.contiguous(), field, self.edge, pixel_format, swap_rb=self.swap_rb, align_corners=self.align_corners,
                                 mode=self.interpolation)
            if keep:
                if (s + halo_left) in cutset or (s == 0 and keep_from is None):
                    init, src = cur.contiguous()[0], True   # a scene's first frame: its own source, as the warp would write it
                elif prev is not None:
                    init, src = prev, False
                else:   # the caller's history: possibly written on another stream (run_video's other lane)
                    if _keep_wait is not None:
                        compute.wait_event(_keep_wait)
                    keep_from.record_stream(compute)
                    init, src = keep_from, False
                PF.keep_borders_(warped, field, init, pixel_format, initial_is_source=src, swap_rb=self.swap_rb, align_corners=self.align_corners,
                                 mode=self.interpolation)
                prev = warped[-1]   # (a view: keeps the batch alive until the next one has read it)
            if on_host:
                done = torch.cuda.Event()
                done.record(compute)
                with torch.cuda.stream(d2h):
                    d2h.wait_event(done)
                    out[s:e].copy_(warped, non_blocking=True)
                warped.record_stream(d2h)
                cur.record_stream(compute)
                pending.append(warped)
            else:
                out[s:e].copy_(warped)
        if mosaic:
            if _mosaic_pad is not None:
                return wall, fall
            edges = [0] + [c - halo_left for c in (cuts or ()) if 0 < c - halo_left < T] + [T]
            for a, b in zip(edges[:-1], edges[1:]):   # one scene piece per call: donors never cross a cut
                PF.mosaic_borders_(wall[a:b], fall[a:b], self.mosaic_radius, pixel_format=pixel_format, align_corners=self.align_corners,
                                   mode=self.interpolation, _unfilled=self.mosaic_unfilled[a:b])
            if on_host:
                done = torch.cuda.Event()
                done.record(compute)
                with torch.cuda.stream(d2h):
                    d2h.wait_event(done)
                    out.copy_(wall, non_blocking=True)
                wall.record_stream(d2h)
            else:
                out.copy_(wall)
        if on_host:
            d2h.synchronize()
        return out

    @torch.no_grad()
    def run_video(self, frames, chunk=32, half_size_output=False, frames_are_rgb=False, halo_left=0, halo_right=0, crop=None,
                  output_size=None, in_flight=1, pixel_format="bgr24", scene_cuts=None, scene_threshold=0.25, scene_min_len=16, zoom=None,
                  zoom_speed=0.002, zoom_min=0.5, metrics=None):
        """The whole device side of the reference's ``process()`` loop for one decoded clip: ``frames`` (T, H, W, 3) uint8 as
        cv2 delivers them, in (pinned) host memory or on the device.  Per chunk of ``chunk`` frames: H2D on a side stream,
        gray + INTER_AREA 256x256 window planes computed there from the uploaded frames (so nothing but the uint8 frames
        crosses PCIe and the host does no per-frame image processing), the generator on batched windows, the fused uint8
        resize+warp, optionally the 2x INTER_AREA down-scale of the output (main_new.py:723), D2H on a third stream.  Chunk
        k+1 uploads while chunk k computes; window planes are kept for the whole clip (256 KB per frame), frames per chunk.
        halo_left / halo_right: ``frames`` additionally holds that many real neighbour frames before / after the T frames to
        stabilise (a rank's shard of a longer clip, ``distributed.shard_frames``: up to period//2 each); they only feed the
        windows.  crop = (x_start, x_end, y_start, y_end[, threshold]): the reference's crop window of the OUTPUT frame
        (main_new.py:607-610,729-730: ``samples[int(y_start)+threshold:int(y_end)-threshold, int(x_start)+threshold:
        int(x_end)-threshold]``, applied after the down-scale), sliced on the device so that only the cropped frames cross PCIe;
        the reference's live values (0, 640, 0, 360, threshold 0) are the whole 640x360 frame.  The 3x3 GaussianBlur(sigma=0.2)
        that follows in the reference (:731) is the identity on 8-bit frames and is not run.
        output_size = (width, height): the reference's ``cv2.resize(samples, (640, 360), INTER_AREA)`` for ANY source size
        (main_new.py:723; half_size_output=True is the same thing for a 1280 x 720 source).
        in_flight = 2: consecutive chunks compute on two streams without waiting for each other (one chunk walks the generator's chain of
        small levels while the other's large layers fill the chip: DESIGN.md section 8); for the duration of the call the generator runs one
        queue per forward and, in graph mode, keeps one graph + arena per stream.  Same frames bit for bit as in_flight = 1.
        crop = "auto": the reference's automatic crop (main_new.py:484-606), which cuts away the black wedges the warp's zero padding
        leaves: pass 1 runs the generator once per frame, keeps the clip's fields on the device ((T, 256, 256, 2) fp32: 512 KB per frame,
        on top of the window planes) and fits each frame's homography (``field_homography``) on the same stream; the host then runs the
        window recurrence over the (T, 4) bounds (``auto_crop_window``, the call's one synchronisation); pass 2 uploads host-resident frames
        again (device-resident ones are read in place) and runs only the warp, the output resize and the crop.  Same frames bit for bit as
        crop=auto_crop_window(bounds, (H, W), output (height, width), period).  Needs the whole clip (no halos) and a source of at least
        600 x 300.
        pixel_format = "nv12" / "i420": ``frames`` are packed 4:2:0 (T, H * 3 // 2, W) uint8 as decoders hand them over (H even, W % 4 == 0),
        YUV in and YUV out in the same layout: the window planes are those of the frames' BGR decode (window_planes_yuv: the same fields
        bit for bit), every plane is warped by the field (functional.upsample_grid_sample_yuv420: BT.601 black padding) and resized plane by
        plane (area_resize_yuv).  Output sizes and crop windows must be even; crop="auto" rounds the BGR path's window inward to even.
        frames_are_rgb=True is an error there, and ``swap_rb`` is ignored.
        pixel_format = "p010" / "i010": 10-bit 4:2:0 frames (T, H * 3 // 2, W) uint16, BT.601 limited range, in NV12's / I420's plane order
        (P010: the sample in the high 10 bits of each word, as hardware decoders deliver it; I010 = yuv420p10le: in the low 10 bits), uint16
        out in the same layout.  The window planes are those of the frames' 8-bit reduction (window_planes_yuv16: the fields of the NV12 /
        I420 clip of the reduced samples bit for bit), the warp and the output resize work on the 10-bit values
        (functional.upsample_grid_sample_yuv420_16: black is 64 / 512; area_resize_yuv16); everything else as for NV12 / I420.  A tensor
        whose dtype does not belong to the pixel format is a ValueError.
        pixel_format = "nv16" / "i422" (uint8) and "p210" / "i210" (uint16), 4:2:2 frames (T, 2 * H, W) -- ProRes, XAVC, DNxHR -- and "i444"
        (uint8) / "i410" (uint16), 4:4:4 frames (T, 3 * H, W): everything as for the 4:2:0 format of the same depth and plane order, with chroma
        planes of H x W/2 resp. H x W samples (functional.upsample_grid_sample_yuv; the window planes decode pixel (x, y) with chroma sample
        (x >> cx, y >> cy)).  H even and W % 4 == 0 as for 4:2:0.  Output sizes and crop edges must be multiples of the subsampling per axis:
        4:2:2 x even and y free, 4:4:4 both free; crop="auto" rounds the BGR path's window inward to those multiples.
        scene_cuts: edited footage.  A sorted sequence of indices into ``frames`` (halo frames count; 1 .. len - 1) at which a new scene starts
        (a hard cut), or "auto" to find them.  Windows end at a cut as they end at the clip's ends (the scene's first / last frame repeated)
        and the generator batches restart there (run()), so every scene is stabilised as a clip of its own, inside the one chunk pipeline;
        crop="auto" applies the reference's end rule per scene and carries its one window across the cuts (auto_crop_window).  "auto": the
        upload stream also runs ``scene_scores`` over each chunk's planes (plus the previous chunk's last one) and copies the scores to
        pinned host memory; before a chunk is issued the host waits for the upload that holds the last plane its windows reach -- one wait
        per chunk on the UPLOAD stream, never on a compute lane -- and extends the cut list with ``find_scene_cuts``' causal rule
        (scene_threshold, scene_min_len).  Only hard cuts are found: a dissolve or a fade stays one scene, as today.  A shard (non-zero
        halo) that detects on its own slice has no history before its halo and may place scene_min_len differently from the whole clip:
        sharded hosts compute ``scene_scores`` per shard, gather, call ``find_scene_cuts`` once and pass explicit lists.  The cuts used are
        left in ``self.scene_cuts``.  None (the default): one scene, every path as without the argument.
        VideoStabilizer(borders="keep"): the field of view is kept instead of cropped -- an output pixel the current frame does not cover (a
        tap of the warp outside the source) keeps the value the previous output frame of its scene had there, and a scene's first frame
        starts from its own source, so no wedge ever shows the pad colour (functional.keep_borders_ has the definition).  The pass runs on
        the warped frames BEFORE the output resize and the crop; each chunk starts from the previous chunk's last warped frame (the tensor
        is kept alive, not copied), and with in_flight > 1 a chunk's first pass waits for an event recorded behind the previous chunk's last
        pass on the other lane -- generator and warp stay unordered between the lanes, and the frames are those of in_flight = 1 bit for
        bit.  Cuts reset the history ("auto" needs no extra wait: a chunk's cuts are known before it is issued).  An explicit crop,
        output_size, half_size_output, halos and host or device input work as before; a shard with halo_left > 0 has no history, starts its
        first frame from that frame's source and does not promise the unsharded clip's bytes in its wedges; crop="auto" is a ValueError
        (it removes what "keep" fills).
        VideoStabilizer(borders="mosaic", mosaic_radius=R): an uncovered pixel takes its value from the temporally nearest stabilised frame of
        its scene that covers it, at most R frames into the past or the FUTURE (functional.mosaic_borders_ has the definition): nothing is
        older than R frames, and chunking does not change a byte.  A chunk is finished one chunk late: chunk c is warped with black borders
        and its fields are kept; then chunk c-1 is filled -- its donors are the last R warped frames of chunk c-2 and the first R of chunk c,
        copied beside it into one buffer, each call cut at the scene limits -- and goes through the output resize, the crop and the copy out
        as usual; the last chunk is finished after the loop.  About two chunks plus 2 R frames and their fields stay on the device.
        scene_cuts (a list or "auto": a chunk's cuts are known before it is issued), output_size, half_size_output, an explicit crop,
        rigidity (coverage uses the field that warped), every integer pixel_format, both interpolations, halos and host or device input work
        as with "black"; a shard's first and last R frames do not promise the unsharded clip's bytes in their wedges (halo frames are not
        warped).  ``self.mosaic_unfilled`` (T,) int32 stays on the device.  ValueError: zoom or crop="auto" (they remove what it fills),
        chunk < R (adjacent chunks must suffice), in_flight > 1 (the one-chunk delay across two lanes needs an event design of its own).
        zoom: zoom to fill (vid.stab's ``zoom`` / ``optzoom``) -- the third answer to the wedges: the output keeps the size that was asked for,
        and shows a window of the stabilised frame enlarged to it.  The zoom is composed into each frame's FIELD (functional.zoom_fields, one
        small launch per batch) and the warp that follows resamples the source once, as without a zoom; windows are fractional, also for the
        YUV formats.  A float k in (0, 1]: the centred window of that fraction of the frame, in the single pass, through ``run(zoom=)``; 1.0
        gives the frames of zoom=None.  "auto": pass 1 is crop="auto"'s (fields and bounds stay on the device); the clip's one window is
        ``zoom_window(auto_crop_window(bounds, (H, W), None, period, cuts), (H, W))``; pass 2 zooms each chunk's kept fields and warps.
        "adaptive": the same two passes with a window per frame, ``zoom_schedule(bounds, (H, W), zoom_speed, zoom_min, cuts)``: as little
        zoom as each frame needs, changing by at most ``zoom_speed`` of the frame per frame, never below the fraction ``zoom_min``.  The
        windows used are left in ``self.zoom_windows`` (T tuples), and ``self.zoom_uncovered`` is a (T,) int32 device tensor: per frame, the
        nodes of the zoomed field that still sample outside the source (no synchronisation: read it when you need it).  output_size,
        half_size_output, in_flight, scene_cuts, host or device input and every pixel_format work as without a zoom.  ValueError: zoom with
        any crop or with borders="keep"; "auto" / "adaptive" with halos or below the 600 x 300 lattice size; any other string; a float
        outside (0, 1].
        VideoStabilizer(rigidity=r), r > 0: rigid warp mode -- every frame's field is pulled towards the homography fitted to it
        (functional.rigid_fields; 1 = the homography alone: no local breathing or wobble, and no parallax correction either).  The single-pass
        paths do it per batch inside run(): generator, fit, blend, [zoom,] warp, [keep].  The two-pass paths (crop="auto", zoom="auto" /
        "adaptive") already fit M on the raw field in pass 1; they then blend the kept fields in place on the same stream, and pass 2 is
        unchanged.  The bounds stay those of the RAW fit: M is by construction the rigid part of the raw field and of any blend of the field
        with P, so a refit of the blended field returns M up to the fit's sampling (at rigidity 1 the four bounds move by 3e-4 pixel or
        less: INTEGRATION.md, tests/test_rigid_ref_cpu.py).  Every pixel_format, interpolation, borders, crop, zoom, in_flight and halo works
        as without it; a source below the fit's 600 x 300 lattice is a ValueError.  ``self.rigid_residual`` (T,) float32 -- per frame, the
        largest distance in source pixels between the generator's field and its homography: the number to choose the setting by -- and
        ``self.rigid_unfit`` (T,) int32 -- the nodes that kept the raw field because no homography applied to them -- are left on the device
        (no synchronisation: read them when you need them); both are None at rigidity 0, which takes no new path.
        VideoStabilizer(edge="clamp" | "mirror"): where a frame's field samples outside the source, the source itself is continued beyond its
        rim -- the edge sample repeated, or the picture reflected about it (functional.edge_borders_ has the definition; ffmpeg deshake's
        ``edge``, OpenCV's BORDER_REPLICATE / BORDER_REFLECT_101) -- instead of blended towards the pad colour.  One more launch behind every
        warp, before the output resize and the crop, reading the chunk's own source frames and the field that warped; no other frame is read,
        so in_flight, halos (a shard needs no history: given the same fields its bytes are the unsharded clip's, as with "pad"), scene_cuts,
        zoom, explicit and automatic crops, rigidity and every integer pixel_format work as with edge="pad", the default, under which every
        path is as it was.  With borders="mosaic" the pass runs
        before the mosaic fill: donors win, and exactly the positions ``mosaic_unfilled`` counts show the edge fill.  borders="keep" with an
        edge is a ValueError at construction (keep never shows the pad colour); float frames are a ValueError.
        metrics (None: what VideoStabilizer(metrics=) said; True / False for this call): measure the clip.  The window planes of every WARPED
        chunk -- what the viewer sees: after keep, mosaic, edge, zoom and rigidity, before the output resize and the crop, in the output's own
        channel order -- are computed on the chunk's lane into one (T, 256, 256) buffer (256 KB per frame, as much again as the input planes);
        once every lane has joined, ``global_motion`` runs once over the input planes of the T core frames and once over the output planes.
        A source of at least 600 x 300 also keeps every frame's raw ``field_homography`` fit (the two-pass paths and rigidity > 0 have it
        already; otherwise one small launch per batch).  Left on the device, no synchronisation: ``self.motion_in`` / ``self.motion_out`` (T, 4)
        float64 and ``self.motion_inliers_in`` / ``self.motion_inliers_out`` (T,) int32; None without metrics.  ``stability_report()`` turns
        them into the paper's stability, cropping and distortion.  The frames are those of metrics=False bit for bit; halos (a shard reports
        its own T frames), scene_cuts, in_flight, every pixel_format, interpolation, borders, edge, zoom and crop mode work as without it.
        VideoStabilizer(smooth=sigma), sigma > 0 frames: path smoothing.  Each frame's field is regressed from that frame's own window, and
        nothing makes consecutive OUTPUT frames move smoothly; this measures what the fields leave and folds it back into them.  The call
        takes the two-pass route, also without a crop or zoom.  Once pass 1 has joined, on the caller's stream: the T core input planes are
        warped by the kept fields (after rigidity; ``functional.grid_sample``, one (T, 256, 256) buffer); ``global_motion(...,
        pixel_scale=(W / 256, H / 256))`` measures the motion left between them, in frame pixels; ``smooth_path`` under the call's cuts gives
        every frame's correction D; ``functional.compose_fields`` folds it into the kept fields chunk by chunk; and, for a source of at
        least 600 x 300, ``field_homography`` is fitted again on the composed fields, so that the bounds, crop="auto", zoom="auto" /
        "adaptive" and the report's cropping and distortion describe the field that warps.  Pass 2 is unchanged: one resampling of the
        source.  With a generator that returns the identity this is a complete classical stabiliser.  Left on the device, no synchronisation,
        None at smooth = 0: ``self.smooth_motion`` (T, 4) float64 and ``self.smooth_inliers`` (T,) int32, ``self.smooth_path`` (T, 4),
        ``self.smooth_correction`` (T, 6) float64 and ``self.smooth_uncovered`` (T,) int32 (the composed fields' nodes that sample outside the
        source).  A pair no similarity could be fitted to counts as no motion.  Every pixel_format, interpolation, edge, crop, zoom,
        rigidity, in_flight and scene_cuts works as without it.  ValueError: halos (a shard cannot see the scene's path), borders="keep" or
        "mosaic" (they have no second pass).
        VideoStabilizer(smooth=sigma, rolling_shutter=r), r != 0: rolling-shutter correction inside the same composition.  r in [-1, 1] is the
        share of the frame interval that the readout from the top row to the bottom row takes (negative: bottom to top).  ``shutter_rates``
        of the measured motion, under the call's cuts, gives every frame's forward and backward velocity; ``compose_fields(rates=,
        rolling_shutter=r)`` takes, per field node, that velocity times the time offset of the node's row out of the position that D gives.
        The refit, and with it crop, zoom and the report, see the corrected field.  ``self.shutter_rates`` (T, 2, 4) float64 is left on the
        device, no synchronisation; None at r = 0.  First order in the time offset, a linear path between frames, the row taken from the
        frame that the motion was measured on (INTEGRATION.md has the model and its caveats); not validated on real footage.
        VideoStabilizer(smooth=sigma, rolling_shutter="auto", shutter_max_se=0.02): r estimated from the clip.  The measurement keeps its
        blocks, ``estimate_rolling_shutter`` regresses their vectors on the row share times the camera's acceleration under the call's
        cuts, and the four numbers (r_hat, se, D, blocks) are read to the host: one 32-byte read, under "auto" only, at which the host
        waits for pass 1.  r = clamp(r_hat, -1, 1) when r_hat is finite and se <= shutter_max_se, else 0.0 (no correction: a still clip,
        a steady pan, fewer than 4 frames); from there on everything is the fixed-r path with that number, bit for bit.  se is a gate,
        not an error bar, and 0.02 a judgement that no footage here can fit.  ``self.shutter_estimate`` (4,) float64 on the device and
        ``self.rolling_shutter_used``, a float; both None otherwise.  The vectors are measured on the planes as the fields warp them:
        what the generator's field already took out of the skew is not seen.
        VideoStabilizer(wobble=sigma), sigma in (0, 5] frames: wobble suppression.  The local, per-pixel part of the field changes from frame
        to frame, which reads as wobble or "jello"; rigidity removes that part and with it the parallax and lens correction a per-pixel field
        exists for.  This low-passes it along time instead (``functional.wobble_fields`` has the definition): per node, the field minus the
        frame's fitted homography is averaged over +-ceil(3 sigma) frames of its scene under a Gaussian, and the homography's own position
        is added back.  The call takes the two-pass route, also without a crop, zoom or smooth; pass 1 fits M on the raw field.  Once pass
        1 has joined, on the caller's stream: the kept fields (after the in-place rigidity blend) are filtered under the call's cuts into a
        second buffer that replaces them -- another 512 KB per frame for the duration of the call; ``field_homography`` is fitted again on
        the result, so that the bounds, crop="auto", zoom="auto" / "adaptive" and the report describe the field that warps (under smooth the
        one refit is the one behind its composition); smooth's measurement follows, so it sees the filtered fields.  Pass 2 is unchanged.
        Left on the device, no synchronisation, None at wobble = 0: ``self.wobble_removed`` (T,) float32 -- per frame, the largest distance
        in source pixels by which the filter moved a node: the number to choose sigma by -- and ``self.wobble_unfit`` (T,) int32, the nodes
        that kept their value.  The filter acts at fixed output positions, so a real, fast change of parallax is smoothed too; nothing
        was validated on real footage.  Every pixel_format, interpolation, edge, crop, zoom, rigidity, smooth, in_flight and scene_cuts
        works as without it.  ValueError: halos, borders="keep" or "mosaic" (no second pass), a source below the fit's 600 x 300 lattice.
        ``run()`` does not take it.
        VideoStabilizer(smooth=sigma, max_crop=c, limit_levels=16, limit_relax=None), c in [0, 0.5]: crop-bounded smoothing (vid.stab's
        ``maxshift`` / ``maxangle``, OpenCV videostab's trim ratio, Warp Stabilizer's "crop less / smooth more").  c is the share of the
        frame, per axis, that the viewer is prepared to lose: the centred window of the fraction 1 - c -- the one zoom=1 - c shows -- stays
        covered by the source.  Between ``smooth_path`` (and ``shutter_rates``) and the composition, on the caller's stream, ``limit_path``
        reads the kept fields in place (after rigidity and wobble), finds per frame the largest of limit_levels + 1 shares of the correction
        under which no node of the window's cells samples outside the source -- ``compose_fields``' own node function, so it holds for
        per-pixel fields and the rolling-shutter composition alike -- and eases the share by at most limit_relax per frame inside each
        scene (None: 1 / ceil(3 sigma), a judgement that no footage here can fit, like zoom_speed; never across a cut).  What is composed,
        refitted, cropped and zoomed is the limited correction.  Left on the device, no synchronisation, None at max_crop=None, which
        takes no new path: ``self.limit_strength`` (T,) float64 in [0, 1], ``self.limit_need`` (T,) int32 (the raw level; -1: the field
        alone does not cover the window), ``self.limit_uncovered`` (T,) int32 (the window's nodes that still sample outside under the
        correction that was composed: the eased share lies between grid levels, where feasibility is not proven -- read it),
        ``self.smooth_correction_unlimited`` (T, 6), what ``smooth_path`` returned; ``self.smooth_correction`` is then the limited D.  It
        bounds the correction and nothing else -- not the generator's own field -- and works with every pixel_format, interpolation,
        edge, crop, zoom, rigidity, wobble, rolling_shutter, in_flight, scene_cuts and metrics.  ValueError: max_crop without smooth > 0.
        Returns (T, H, W, 3) -- or (T, H/2, W/2, 3) / (T, height, width, 3), or the crop window of it -- uint8 on the inputs' side; for YUV
        (T, oh * 3 // 2, ow) of the output (or crop window) size oh x ow."""
        half = self.period // 2
        if not (0 <= halo_left <= half and 0 <= halo_right <= half):
            raise ValueError("halo must be within [0, %d]" % half)
        n_all = frames.shape[0]
        T = n_all - halo_left - halo_right
        if T < 0:
            raise ValueError("frames holds %d frames, fewer than the halos %d + %d" % (n_all, halo_left, halo_right))
        on_host = not frames.is_cuda
        dev = self.device
        fmt = PF.frame_format(pixel_format, frames, "run_video")   # (from here on the format is this record)
        yuv = fmt.packed   # output sizes and crop edges: multiples of the subsampling per axis (4:2:0: even)
        mx, my = fmt.multiples if yuv else (1, 1)
        h, w = fmt.frame_shape(frames)[1:]
        if yuv and frames_are_rgb:
            raise ValueError("run_video: frames_are_rgb has no meaning for %s frames" % pixel_format)
        if output_size is not None and half_size_output:
            raise ValueError("run_video: give output_size or half_size_output, not both")
        if output_size is not None:
            ow, oh = int(output_size[0]), int(output_size[1])
            if not (0 < ow <= w and 0 < oh <= h):
                raise ValueError("run_video: output_size %s must not exceed the %d x %d source (INTER_AREA down-scaling)" % (tuple(output_size), w, h))
        else:
            oh, ow = (h // 2, w // 2) if half_size_output else (h, w)
        if yuv and (oh % my or ow % mx):
            if fmt.chroma == 0:
                raise ValueError("run_video: the %s output size %d x %d must be even" % (pixel_format, ow, oh))
            raise ValueError("run_video: the %s output size %d x %d must be a multiple of %d x %d" % (pixel_format, ow, oh, mx, my))
        auto = isinstance(crop, str)
        if auto:
            if crop != "auto":
                raise ValueError("crop must be None, \"auto\" or (x_start, x_end, y_start, y_end[, threshold])")
            if halo_left or halo_right:
                raise ValueError("run_video: crop=\"auto\" needs the whole clip (a shard cannot see the clip's crop recurrence): gather "
                                 "the shards' field_homography bounds and pass crop=auto_crop_window(...)")
            if self.borders in ("keep", "mosaic"):
                raise ValueError("run_video: crop=\"auto\" removes the wedges that borders=\"%s\" fills: choose one" % self.borders)
            _check_lattice(h, w)
        self.zoom_windows = self.zoom_uncovered = None
        self.rigid_residual = self.rigid_unfit = None
        self.mosaic_unfilled = None
        self.motion_in = self.motion_out = self.motion_inliers_in = self.motion_inliers_out = self._report = None
        metrics = self.metrics if metrics is None else bool(metrics)
        if self.edge != "pad" and frames.dtype not in (torch.uint8, torch.uint16):
            raise ValueError("run_video: edge=%r is for the integer pixel formats (uint8 / uint16 frames), got %s" % (self.edge, frames.dtype))
        mosaic, radius = self.borders == "mosaic", self.mosaic_radius
        if mosaic:
            if frames.dtype not in (torch.uint8, torch.uint16):
                raise ValueError("run_video: borders=\"mosaic\" is for the integer pixel formats (uint8 / uint16 frames), got %s" % (frames.dtype,))
            if max(1, int(in_flight)) > 1:
                raise ValueError("run_video: borders=\"mosaic\" finishes a chunk one chunk late, which across two lanes needs an event design of "
                                 "its own: use in_flight=1")
            if int(chunk) < radius:
                raise ValueError("run_video: chunk=%d is shorter than mosaic_radius=%d: a chunk's donors must lie in the adjacent chunks" % (chunk, radius))
        rigid = self.rigidity > 0.0
        if rigid:
            _check_lattice(h, w, "rigidity > 0")
        zmode = None
        if zoom is not None:
            if crop is not None:
                raise ValueError("run_video: zoom fills the frame that a crop would cut: give zoom or crop, not both")
            if self.borders in ("keep", "mosaic"):
                raise ValueError("run_video: zoom removes the wedges that borders=\"%s\" fills: choose one" % self.borders)
            if isinstance(zoom, str):
                if zoom not in ("auto", "adaptive"):
                    raise ValueError("zoom must be None, a fraction in (0, 1], \"auto\" or \"adaptive\", got %r" % (zoom,))
                if halo_left or halo_right:
                    raise ValueError("run_video: zoom=%r needs the whole clip (a shard cannot see the clip's bounds): gather the shards' "
                                     "field_homography bounds and pass windows to run(zoom=)" % (zoom,))
                _check_lattice(h, w, "zoom=%r" % (zoom,))
                zmode = zoom
            else:
                try:
                    zk = float(zoom)
                except (TypeError, ValueError):
                    raise ValueError("zoom must be None, a fraction in (0, 1], \"auto\" or \"adaptive\", got %r" % (zoom,)) from None
                if not 0.0 < zk <= 1.0:
                    raise ValueError("zoom: the fraction of the frame must lie in (0, 1], got %r" % (zoom,))
                zmode = "fixed"
                zwin = _centred_window(zk, h, w)
        smoothing = self.smooth > 0.0
        self.smooth_motion = self.smooth_inliers = self.smooth_path = self.smooth_correction = self.smooth_uncovered = None
        self.shutter_rates = self.shutter_estimate = self.rolling_shutter_used = None
        rs = _check_shutter(self.rolling_shutter, "run_video")   # (the attributes can be set after construction)
        max_se = _check_max_se(self.shutter_max_se, "run_video")
        if rs != 0.0 and not smoothing:
            raise ValueError("run_video: rolling_shutter=%r needs smooth > 0" % (self.rolling_shutter,))
        max_crop, limit_levels, limit_relax = _check_limit(self.max_crop, self.limit_levels, self.limit_relax, self.smooth, "run_video")
        self.limit_strength = self.limit_need = self.limit_uncovered = self.smooth_correction_unlimited = None
        if max_crop is not None and not smoothing:   # (the attributes can be set after construction)
            raise ValueError("run_video: max_crop=%r needs smooth > 0" % (self.max_crop,))
        if smoothing:
            if halo_left or halo_right:
                raise ValueError("run_video: smooth > 0 needs the whole clip (a shard cannot see the scene's path)")
            if self.borders in ("keep", "mosaic"):
                raise ValueError("run_video: smooth > 0 warps in a second pass, which borders=\"%s\" does not have yet" % self.borders)
        wob = PF._check_wobble(self.wobble, "run_video", zero_ok=True)   # (the attribute can be set after construction)
        self.wobble_removed = self.wobble_unfit = None
        if wob > 0.0:
            if halo_left or halo_right:
                raise ValueError("run_video: wobble > 0 needs the whole clip (a shard cannot see its neighbours' fields)")
            if self.borders in ("keep", "mosaic"):
                raise ValueError("run_video: wobble > 0 warps in a second pass, which borders=\"%s\" does not have yet" % self.borders)
            _check_lattice(h, w, "wobble > 0")
        lattice = h >= 300 and w >= 600   # the homography fit's
        two_pass = auto or zmode in ("auto", "adaptive") or smoothing or wob > 0.0   # pass 1: fields and bounds; the host's decision; pass 2: the warp
        detect = isinstance(scene_cuts, str)
        if detect and scene_cuts != "auto":
            raise ValueError("scene_cuts must be None, \"auto\" or a sorted sequence of frame indices, got %r" % (scene_cuts,))
        cuts = [] if detect or scene_cuts is None else _check_cuts(scene_cuts, n_all, "run_video")
        self.scene_cuts = cuts

        def crop_window(crop):
            cy0, cy1, cx0, cx1 = 0, oh, 0, ow
            if crop is not None:
                if len(crop) not in (4, 5):
                    raise ValueError("crop must be (x_start, x_end, y_start, y_end[, threshold])")
                th = int(crop[4]) if len(crop) == 5 else 0
                cx0, cx1, cy0, cy1 = int(crop[0]) + th, int(crop[1]) - th, int(crop[2]) + th, int(crop[3]) - th
                if not (0 <= cx0 < cx1 <= ow and 0 <= cy0 < cy1 <= oh):
                    raise ValueError("crop window x [%d, %d) y [%d, %d) does not lie inside the %d x %d output frame" % (cx0, cx1, cy0, cy1, ow, oh))
                if yuv and ((cx0 | cx1) % mx or (cy0 | cy1) % my):
                    if fmt.chroma == 0:
                        raise ValueError("crop window x [%d, %d) y [%d, %d) of %s frames must have even edges" % (cx0, cx1, cy0, cy1, pixel_format))
                    raise ValueError("crop window x [%d, %d) y [%d, %d) of %s frames must have edges that are multiples of %d (x) and %d (y)"
                                     % (cx0, cx1, cy0, cy1, pixel_format, mx, my))
            return cy0, cy1, cx0, cx1

        def alloc_out():
            oshape = _frames_shape(fmt, T, cy1 - cy0, cx1 - cx0)
            return torch.empty(oshape, dtype=frames.dtype, pin_memory=True) if on_host else torch.empty(oshape, dtype=frames.dtype, device=dev)
        cy0, cy1, cx0, cx1 = crop_window(None if auto else crop)
        out = None if auto and T > 0 else alloc_out()
        if T == 0:
            return out
        compute = torch.cuda.current_stream(dev)
        up, down = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        in_flight = max(1, int(in_flight))
        if rigid:   # (before the lanes fork from the caller's stream: every lane writes its chunks' slices)
            rres = torch.empty((T,), device=dev, dtype=torch.float32)
            runf = torch.empty((T,), device=dev, dtype=torch.int32)
        mhom = mbounds = None
        if metrics:   # (also before the fork) the output planes; below the fit's lattice size cropping and distortion are not reported
            planes_out = torch.empty((T, 256, 256), device=dev, dtype=torch.float32)
            out_rgb = (bool(frames_are_rgb) != self.swap_rb) if not yuv else False   # the warp's swap_rb turns the channel order round
            if lattice and not two_pass:   # (the two-pass paths keep their own fit)
                mhom = torch.empty((T, 9), device=dev, dtype=torch.float64)
                mbounds = torch.empty((T, 4), device=dev, dtype=torch.float32)
        # (the lanes live as long as this object: the generator keeps an arena / a graph per STREAM, and torch's allocator a pool per stream)
        # The caller's stream is lane 0: the runtime deals streams to a handful of hardware queues, and a lane that shares its queue with
        # the upload or the download stream waits behind their copies (two NEW lanes beside up / down: 1 744 -> 1 291 frames/s).
        while len(self._lanes) < in_flight - 1:
            self._lanes.append(torch.cuda.Stream(dev))
        lanes = [compute] + self._lanes[:in_flight - 1]
        mod = getattr(self.net, "module", self.net)
        restore = None
        if in_flight > 1:
            restore = (mod._graph_mode, mod._graph_alias, getattr(mod, "_graph_per_stream", False), mod.two_queues)
            mod.two_queues = False   # two forwards that both fork into the device's one side queue would serialise there
            if mod._graph_mode:
                mod.enable_graph(True, mod._graph_alias, per_stream=True)
            for lane in lanes[1:]:
                lane.wait_stream(compute)
        gray_all = torch.empty((n_all, 256, 256), device=dev, dtype=torch.float32)
        if zmode is not None:
            zunc = torch.empty((T,), device=dev, dtype=torch.int32)
        if two_pass:
            fields = torch.empty((T, 256, 256, 2), device=dev, dtype=torch.float32)
            hom = torch.empty((T, 9), device=dev, dtype=torch.float64)
            bounds = torch.empty((T, 4), device=dev, dtype=torch.float32)
        # chunk bounds in the index space of `frames`: the first / last chunk carry the halo frames with them
        chunks = [(s if s > halo_left else 0, min(halo_left + T, s + chunk) if s + chunk < halo_left + T else n_all)
                  for s in range(halo_left, halo_left + T, chunk)]
        up.wait_stream(compute)   # gray_all was allocated on the compute stream

        def upload(c):
            s, e = chunks[c]
            with torch.cuda.stream(up):
                buf = frames[s:e].to(dev, non_blocking=True) if on_host else frames[s:e]
                _window_planes(buf, fmt, 256, gray_all[s:e], "run_video", frames_are_rgb)
                ev = torch.cuda.Event()
                ev.record(up)
                if detect:   # same stream: ordered behind the planes (and behind the previous chunk's, whose last plane it reads)
                    s0 = max(s - 1, 0)
                    scores_h[s:e].copy_(scene_scores(gray_all[s0:e])[s - s0:], non_blocking=True)
                    scored[c] = torch.cuda.Event()
                    scored[c].record(up)
            return buf, ev

        def detect_cuts(need):
            """extends the cut list over the planes 0 .. need-1 (the host waits for the upload that scored plane need-1)"""
            nonlocal decided
            k = next(k for k, (s, e) in enumerate(chunks) if e >= need)
            t0 = time.perf_counter()
            scored[k].synchronize()
            self.scene_wait_s += time.perf_counter() - t0
            last = cuts[-1] if cuts else 0
            first = max(decided, 1)
            for t, v in enumerate(scores_h[first:need].tolist(), first):
                if v > scene_threshold and t - last >= scene_min_len:   # find_scene_cuts' rule, continued
                    cuts.append(t)
                    last = t
            decided = max(decided, need)

        def finish(warped, buf, s, e, lane):
            """output resize + crop of the warped core frames s .. e-1 (output positions) on `lane`, and their way to `out`"""
            if metrics:   # the planes of what the viewer sees, at the warp's size
                _window_planes(warped, fmt, 256, planes_out[s:e], "run_video", out_rgb)
            if (oh, ow) != (h, w):
                warped = _output_resize(warped, fmt, (ow, oh), half_size_output)
            if crop is not None:
                warped = _crop(warped, fmt, oh, ow, cy0, cy1, cx0, cx1)
            if on_host:
                buf.record_stream(lane)
                done = torch.cuda.Event()
                done.record(lane)
                with torch.cuda.stream(down):
                    down.wait_event(done)
                    out[s:e].copy_(warped, non_blocking=True)
                warped.record_stream(down)
            else:
                out[s:e].copy_(warped)
        pend = None   # borders="mosaic": the chunk that waits for its successor -- (warped, fields, cs, ce, buf, valid frames of the head pad)
        if mosaic:
            unf = torch.empty((T,), device=dev, dtype=torch.int32)

        def mosaic_step(new, lane):
            """chunk `new` = (warped, fields, cs, ce, buf), both buffers with `radius` spare frames at either end, has been warped (None: the
            clip is over): the waiting chunk takes its first frames as donors, is filled scene by scene and finished; `new` takes the
            waiting chunk's last frames and waits in its turn.  (Filled frames are as good donors as the warp's own.)"""
            nonlocal pend
            R = radius
            if pend is not None:
                pw, pf, ps, pe, pbuf, nt = pend
                nh = 0
                if new is not None:
                    nh = min(R, new[3] - new[2])
                    pw[R + pe - ps:R + pe - ps + nh].copy_(new[0][R:R + nh])
                    pf[R + pe - ps:R + pe - ps + nh].copy_(new[1][R:R + nh])
                lo, hi, off = ps - nt, pe + nh, R - ps   # the frames the buffer holds (index space of `frames`); frame g is at g + off
                edges = [halo_left] + [t for t in cuts if halo_left < t < halo_left + T] + [halo_left + T]
                for a, b in zip(edges[:-1], edges[1:]):
                    fa, fb = max(a, ps), min(b, pe)
                    if fa < fb:
                        da, db = max(a, lo), min(b, hi)
                        PF.mosaic_borders_(pw[da + off:db + off], pf[da + off:db + off], R, fa - da, fb - da, pixel_format=pixel_format,
                                           align_corners=self.align_corners, mode=self.interpolation, _unfilled=unf[fa - halo_left:fb - halo_left])
                finish(pw[R:R + pe - ps], pbuf, ps - halo_left, pe - halo_left, lane)
            if new is not None:
                nt = 0
                if pend is not None:
                    nt = min(R, pe - ps)
                    new[0][R - nt:R].copy_(pw[R + pe - ps - nt:R + pe - ps])
                    new[1][R - nt:R].copy_(pf[R + pe - ps - nt:R + pe - ps])
                pend = tuple(new) + (nt,)
            else:
                pend = None
        staged, uploaded = {}, 0
        keep = self.borders == "keep"
        carry, carried = None, None   # borders="keep": the last warped (pre-resize) frame so far, and the event behind the pass that made it
        if detect:
            scores_h = torch.empty((n_all,), dtype=torch.float32, pin_memory=True)
            scored, decided = {}, 0
            self.scene_wait_s = 0.0   # host time spent in those waits (tools/scene_cuts_bench.py)
        try:
            for c, (s, e) in enumerate(chunks):
                lane = lanes[c % len(lanes)]
                # a chunk's windows reach `half` frames past its end: every chunk that holds one of those frames must be on the
                # device (and its planes computed) first; one chunk further ahead keeps the upload stream busy during this compute
                need = min(n_all, e + half)
                while uploaded < len(chunks) and (chunks[uploaded][0] < need or uploaded <= c + 1):
                    staged[uploaded] = upload(uploaded)
                    uploaded += 1
                for k in range(c, uploaded):
                    if chunks[k][0] < need:
                        lane.wait_event(staged[k][1])
                # (planes of EARLIER chunks that this one's windows reach back into were produced before staged[c]'s event on the same stream)
                buf, ev = staged.pop(c)
                # core frames of this chunk (the halo frames at the clip's ends are uploaded with it but not stabilised)
                cs, ce = max(s, halo_left), min(e, halo_left + T)
                hl, hr = min(half, cs), min(half, n_all - ce)
                if detect:
                    detect_cuts(ce + hr)
                # the cuts inside this chunk's slice of the planes, in the slice's index space (None without cuts: the path as it was)
                sc = [t - (cs - hl) for t in cuts if cs - hl < t < ce + hr] or None
                with torch.cuda.stream(lane):
                    if two_pass:   # pass 1: fields and per-frame bounds only (no halos here: core frames = output positions)
                        self._fields(gray_all[cs - hl:ce + hr], hl, hr, fields[cs:ce], sc)
                        if not smoothing or rigid or wob > 0.0:   # (smoothing fits the fields it composes, below; the blend and the wobble
                            #                                         filter need the raw fit)
                            _field_homography(fields[cs:ce], h, w, hom[cs:ce], bounds[cs:ce])
                        if rigid:   # the kept fields, in place; the bounds stay the raw fit's
                            PF._field_rigid(fields[cs:ce], hom[cs:ce], (h, w), self.rigidity, fields[cs:ce], rres[cs:ce], runf[cs:ce])
                        continue
                    rstats = (rres[cs - halo_left:ce - halo_left], runf[cs - halo_left:ce - halo_left]) if rigid else None
                    mh = (mhom[cs - halo_left:ce - halo_left], mbounds[cs - halo_left:ce - halo_left]) if mhom is not None else None
                    if mosaic:   # warped with black borders; the chunk before it is filled and finished
                        wall, fall = self.run(gray_all[cs - hl:ce + hr], buf[cs - s:ce - s], halo_left=hl, halo_right=hr, pixel_format=pixel_format,
                                              scene_cuts=sc, _rigid_stats=rstats, _mosaic_pad=radius, _hom_out=mh)
                        mosaic_step((wall, fall, cs, ce, buf), lane)
                        continue
                    if zmode is not None:   # ("fixed": the one window, in the single pass)
                        warped = self.run(gray_all[cs - hl:ce + hr], buf[cs - s:ce - s], halo_left=hl, halo_right=hr, pixel_format=pixel_format,
                                          scene_cuts=sc, zoom=zwin, _zoom_unc=zunc[cs - halo_left:ce - halo_left], _rigid_stats=rstats, _hom_out=mh)
                    else:
                        warped = self.run(gray_all[cs - hl:ce + hr], buf[cs - s:ce - s], halo_left=hl, halo_right=hr, pixel_format=pixel_format, scene_cuts=sc,
                                          keep_from=carry, _keep_wait=carried, _rigid_stats=rstats, _hom_out=mh)
                    if keep:   # the next chunk's pass (on the other lane, if any) starts from this chunk's last frame: no copy, one event
                        carry = warped[-1]
                        if len(lanes) > 1:
                            carried = torch.cuda.Event()
                            carried.record(lane)
                    finish(warped, buf, cs - halo_left, ce - halo_left, lane)
            if mosaic:
                mosaic_step(None, compute)   # the last chunk
                self.mosaic_unfilled = unf
        finally:
            if restore is not None:
                for lane in lanes[1:]:
                    compute.wait_stream(lane)   # the caller's stream sees every chunk; gray_all and the outputs may be freed behind it
                mod.two_queues = restore[3]
                mod.enable_graph(restore[0], restore[1], per_stream=restore[2])
        if rigid:
            self.rigid_residual, self.rigid_unfit = rres, runf
        if zmode is not None:
            self.zoom_windows, self.zoom_uncovered = [zwin] * T if zmode == "fixed" else None, zunc
        if wob > 0.0:   # every lane has joined the caller's stream: the kept fields (after rigidity) are complete, and so is the cut list
            fields, self.wobble_removed, self.wobble_unfit = PF.wobble_fields(fields, hom, (h, w), wob, scene_cuts=cuts or None, return_stats=True)
            if not smoothing:   # bounds, crop and zoom decisions and the report describe the field that warps (smoothing fits what it composes)
                _field_homography(fields, h, w, hom, bounds)
        if smoothing:   # ... and it measures the filtered fields
            seen = PF.grid_sample(gray_all.unsqueeze(1), fields, align_corners=self.align_corners).squeeze(1)   # the planes as the fields warp them
            if rs == "auto":   # the blocks behind the fit are kept for the estimate: the same launches, the same motion
                self.smooth_motion, self.smooth_inliers, mv, sad, act = global_motion(seen, pixel_scale=(w / 256.0, h / 256.0), return_blocks=True)
                self.shutter_estimate = estimate_rolling_shutter(self.smooth_motion, mv, sad, act, tuple(seen.shape[1:]),
                                                                 pixel_scale=(w / 256.0, h / 256.0), scene_cuts=cuts or None, frame_height=h)
                del mv, sad, act
                r_hat, se = self.shutter_estimate.tolist()[:2]   # the one read of "auto": 32 bytes, and the host waits for pass 1 here
                rs = min(1.0, max(-1.0, r_hat)) if math.isfinite(r_hat) and se <= max_se else 0.0
                self.rolling_shutter_used = rs
            else:
                self.smooth_motion, self.smooth_inliers = global_motion(seen, pixel_scale=(w / 256.0, h / 256.0))
            del seen
            self.smooth_correction, self.smooth_path = smooth_path(self.smooth_motion, self.smooth, scene_cuts=cuts or None)
            self.smooth_uncovered = torch.empty((T,), device=dev, dtype=torch.int32)
            if rs != 0.0:   # the velocity at every frame, from the same measured motion and under the same cuts
                self.shutter_rates = shutter_rates(self.smooth_motion, scene_cuts=cuts or None)
            if max_crop is not None:   # the crop budget: every frame's share of its correction, decided on the kept fields, read in place
                self.smooth_correction_unlimited = self.smooth_correction
                self.smooth_correction, self.limit_strength, self.limit_need, self.limit_uncovered = limit_path(
                    self.smooth_correction, fields, (h, w), 1.0 - max_crop, levels=limit_levels, relax=limit_relax, scene_cuts=cuts or None,
                    rates=self.shutter_rates, rolling_shutter=rs, align_corners=self.align_corners, mode=self.interpolation)
            scratch = torch.empty((min(int(chunk), T),) + tuple(fields.shape[1:]), device=dev, dtype=torch.float32)
            for s in range(0, T, scratch.shape[0]):
                e = min(T, s + scratch.shape[0])
                if rs != 0.0:
                    PF._field_compose_rows(fields[s:e], self.smooth_correction[s:e], self.shutter_rates[s:e], rs, (h, w), self.align_corners,
                                           self.interpolation, scratch[:e - s], self.smooth_uncovered[s:e])
                else:
                    PF._field_compose(fields[s:e], self.smooth_correction[s:e], (h, w), self.align_corners, self.interpolation, scratch[:e - s],
                                      self.smooth_uncovered[s:e])
                fields[s:e].copy_(scratch[:e - s])
                if lattice:   # bounds, crop and zoom decisions and the report describe the field that warps
                    _field_homography(fields[s:e], h, w, hom[s:e], bounds[s:e])
            del scratch
        if zmode in ("auto", "adaptive"):   # (the copy of the bounds to the host waits for pass 1)
            if zmode == "auto":
                self.zoom_windows = [zoom_window(auto_crop_window(bounds, (h, w), None, self.period, scene_cuts=cuts or None), (h, w))] * T
            else:
                self.zoom_windows = zoom_schedule(bounds, (h, w), zoom_speed, zoom_min, scene_cuts=cuts or None)
        if two_pass and zmode is not None:   # (a fixed fraction under smoothing: its one window, in pass 2)
            zcoef = PF.zoom_coefficients(PF._zoom_windows(self.zoom_windows, T, (h, w), "run_video"), (h, w), fields.shape[1:3]).to(dev, non_blocking=True)
        if auto:
            crop = auto_crop_window(bounds, (h, w), (oh, ow), self.period, scene_cuts=cuts or None)   # (the copy to the host waits for pass 1)
            if yuv:   # the BGR path's window, rounded inward to the format's multiples (4:2:0: even edges; 4:4:4: as it is)
                x0, x1, y0, y1 = int(crop[0]), int(crop[1]), int(crop[2]), int(crop[3])
                crop = (x0 + (-x0) % mx, x1 - x1 % mx, y0 + (-y0) % my, y1 - y1 % my)
                if not (crop[1] > crop[0] and crop[3] > crop[2]):
                    raise ValueError("run_video: the even crop window x [%d, %d) y [%d, %d) is empty" % crop)
            cy0, cy1, cx0, cx1 = crop_window(crop)
            out = alloc_out()
        if two_pass:
            # pass 2: [zoom +] warp + output resize + crop with the kept fields; chunk k+1 uploads while chunk k computes

            def fetch(c):
                return _prefetch(frames, chunks[c][0], chunks[c][1], up, dev)
            nxt = fetch(0)
            for c, (s, e) in enumerate(chunks):
                buf, ev = nxt
                if c + 1 < len(chunks):
                    nxt = fetch(c + 1)
                if ev is not None:
                    compute.wait_event(ev)
                fld = fields[s:e]
                if zmode is not None:
                    fld = PF._field_zoom(fld, zcoef[s:e], (h, w), self.align_corners, self.interpolation, torch.empty_like(fld), zunc[s:e])
                warped = PF.warp(buf.contiguous(), fld, fmt, swap_rb=self.swap_rb, align_corners=self.align_corners, mode=self.interpolation)
                if self.edge != "pad":
                    PF.edge_borders_(warped, buf.contiguous(), fld, self.edge, pixel_format, swap_rb=self.swap_rb, align_corners=self.align_corners,
                                     mode=self.interpolation)
                finish(warped, buf, s, e, compute)
        if metrics:   # every lane has joined the caller's stream, and every chunk's planes are behind an event it has waited for
            core = gray_all[halo_left:halo_left + T]
            self.motion_in, self.motion_inliers_in = global_motion(core)
            self.motion_out, self.motion_inliers_out = global_motion(planes_out)
            if two_pass and h >= 300 and w >= 600:
                mhom, mbounds = hom, bounds
            self._report = {"frames": T, "frame_hw": (h, w), "hom": mhom, "bounds": mbounds,
                            "cuts": [c - halo_left for c in cuts if 0 < c - halo_left < T]}
        if on_host:
            down.synchronize()
        return out

    def stability_report(self):
        """The paper's three metrics for the last ``run_video(metrics=True)``; synchronises the device.  Returns a dict:
        ``stability_in`` / ``stability_out``: ``stability_scores`` of ``motion_in`` / ``motion_out`` under the call's scene cuts -- the clip's
        "stability", "translation" and "rotation" and the per-scene list "scenes"; steadier is closer to 1.
        ``cropping``: {"per_frame", "mean", "min"} -- per frame, the share of the frame that the raw fit's ``bounds`` rectangle (top, bottom,
        left, right: ``field_homography``), clipped to the frame, leaves.
        ``distortion``: {"per_frame", "mean", "min"} -- per frame, sigma_min / sigma_max of the Jacobian of the fitted homography M at the frame
        centre, expressed in pixels rather than in normalised coordinates -- output pixels per source pixel, under the generator's
        coordinate convention -- so that a 16:9 frame's aspect does not count as distortion.
        The paper takes the ratio of the affine part's eigenvalues; singular values are used here because a shear has both eigenvalues
        equal to 1 and would pass as undistorted.  1 = a similarity.
        Both are None for a source below the fit's 600 x 300 lattice size; a frame without a fit is NaN in "per_frame" and is left out of
        "mean" and "min" (NaN when no frame has one).
        ``unfit_pairs_in`` / ``unfit_pairs_out``: the pairs inside a scene (the pair at a cut does not count) that ``global_motion`` could
        not fit -- NaN rows.
        The scores are pinned on synthetic clips only: no real footage or trained weights were available to validate them."""
        import numpy as np
        rep = self._report
        if rep is None:
            raise RuntimeError("stability_report: the last run_video did not run with metrics=True")
        torch.cuda.synchronize(self.device)
        T, (h, w), cuts = rep["frames"], rep["frame_hw"], rep["cuts"]
        out = {}
        for side, motion in (("in", self.motion_in), ("out", self.motion_out)):
            m = motion.cpu().numpy()
            out["stability_" + side] = stability_scores(m, cuts or None)
            counted = np.ones(T, bool)
            counted[[0] + cuts] = False
            out["unfit_pairs_" + side] = int((np.isnan(m).any(1) & counted).sum())

        def summary(v):
            ok = v[np.isfinite(v)]
            return {"per_frame": v.tolist(), "mean": float(ok.mean()) if len(ok) else float("nan"), "min": float(ok.min()) if len(ok) else float("nan")}
        if rep["hom"] is None:
            out["cropping"] = out["distortion"] = None
            return out
        b = rep["bounds"].to("cpu", torch.float64).numpy()
        hh = np.clip(np.minimum(b[:, 1], float(h)) - np.maximum(b[:, 0], 0.0), 0.0, None)
        ww = np.clip(np.minimum(b[:, 3], float(w)) - np.maximum(b[:, 2], 0.0), 0.0, None)
        out["cropping"] = summary(hh * ww / float(h * w))
        M = rep["hom"].cpu().numpy().reshape(T, 3, 3)
        # a unit of the field's value in source pixels, under the generator's coordinate convention (the warp's: x = ((v + 1) w - 1) / 2, or
        # (v + 1) (w - 1) / 2 with align_corners); M's own output is u = 2x/w - 1
        sx, sy = (0.5 * (w - 1), 0.5 * (h - 1)) if self.align_corners else (0.5 * w, 0.5 * h)
        ratio = np.full(T, np.nan)
        for t in range(T):
            m = M[t]
            if not np.isfinite(m).all() or m[2, 2] == 0.0:
                continue
            # the Jacobian at the centre (0, 0) of the map (x, y) -> (m0 x + m1 y + m2, m3 x + m4 y + m5) / (m6 x + m7 y + m8), then from
            # normalised coordinates to pixels on both sides
            d = m[2, 2]
            J = (m[:2, :2] - np.outer(m[:2, 2], m[2, :2]) / d) / d
            J = np.diag([0.5 * w, 0.5 * h]) @ J @ np.diag([1.0 / sx, 1.0 / sy])
            sv = np.linalg.svd(J, compute_uv=False)
            if np.isfinite(sv).all() and sv[0] > 0.0:
                ratio[t] = sv[1] / sv[0]
        out["distortion"] = summary(ratio)
        return out
