"""Camera motion of a clip: scene scores, block matching and the similarity fit, the smoothed path, shutter rates and estimate, the crop
budget and the stability metric."""
import ctypes
import math

import torch

from . import functional as PF
from . import hipabi as A
from .framing import _centred_window
from .scenes import _cut_list, _scenes


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
    t, h, w = planes.shape
    return t, h, w, _check_radius(radius, h, w, what)


def _check_radius(radius, h, w, what):
    """The search radius as an int in 1 .. 16 that leaves an h x w plane a 16 x 16 block; ValueError otherwise."""
    radius = int(radius)
    if not 1 <= radius <= 16:
        raise ValueError("%s: radius must be 1 .. 16, got %r" % (what, radius))
    if h - 2 * radius < 16 or w - 2 * radius < 16:
        raise ValueError("%s: a %d x %d plane holds no 16 x 16 block inside a margin of %d" % (what, h, w, radius))
    return radius


def _check_motion(motion, what):
    """``motion`` as ``global_motion`` returns it; ValueError otherwise."""
    if not isinstance(motion, torch.Tensor) or not motion.is_cuda or motion.dtype != torch.float64 or motion.dim() != 2 or motion.shape[1] != 4:
        raise ValueError("%s: motion must be a (T, 4) float64 tensor on the device" % what)


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
    _check_motion(motion, "smooth_path")
    sigma = _check_sigma(sigma, "smooth_path")
    motion = motion.contiguous()
    T = motion.shape[0]
    cuts = _cut_list(scene_cuts, T, "smooth_path")
    d = torch.empty((T, 6), device=motion.device, dtype=torch.float64)
    path = torch.empty((T, 4), device=motion.device, dtype=torch.float64)
    for a, b in (_scenes(T, cuts) if T else []):
        A.check(A.lib().pws_path_smooth(A.ptr(motion[a:b]), b - a, sigma, A.ptr(path[a:b]), A.ptr(d[a:b]), A.current_stream()), "pws_path_smooth")
    return d, path


L1_REACH, L1_WEIGHTS = 0.1, (10.0, 1.0, 100.0)


def _check_l1(reach, weights, what):
    """(reach, weights) of the L1-optimal path checked: ``reach`` a float in (0, 0.5], ``weights`` three positive finite floats; ValueError
    otherwise (NaN included)."""
    try:
        c = float(reach)
    except (TypeError, ValueError):
        raise ValueError("%s: reach must be a share of the frame in (0, 0.5], got %r" % (what, reach)) from None
    if not 0.0 < c <= 0.5:   # (False for NaN)
        raise ValueError("%s: reach must lie in (0, 0.5], got %r" % (what, reach))
    try:
        w = tuple(float(v) for v in weights)
    except (TypeError, ValueError):
        raise ValueError("%s: weights must be three positive finite numbers (w1, w2, w3), got %r" % (what, weights)) from None
    if len(w) != 3 or not all(0.0 < v < math.inf for v in w):
        raise ValueError("%s: weights must be three positive finite numbers (w1, w2, w3), got %r" % (what, weights))
    return c, w


def _l1_bounds(reach, frame_hw, what):
    """The box's half-widths (log scale, angle, x, y) for ``reach`` = c of an H x W frame: (-log(1 - c), c min(H, W) / max(H, W), c W / 2,
    c H / 2) -- each alone moves a frame's rim by the share c of the frame; ValueError for a frame that is not two integers >= 2."""
    try:
        h, w = (int(v) for v in frame_hw)
    except (TypeError, ValueError):
        raise ValueError("%s: frame_hw must be (H, W), got %r" % (what, frame_hw)) from None
    if h < 2 or w < 2:
        raise ValueError("%s: the frame must be at least 2 x 2 pixels, got %d x %d" % (what, w, h))
    return (-math.log(1.0 - reach), reach * min(h, w) / max(h, w), reach * w / 2.0, reach * h / 2.0)


def optimal_path(motion, frame_hw, reach=L1_REACH, weights=L1_WEIGHTS, scene_cuts=None, return_info=False):
    """The L1-optimal camera path (Grundmann, Kwatra, Essa, CVPR 2011; OpenCV videostab's LpMotionStabilizer) in ``smooth_path``'s place
    (csrc/path_l1.hip; include/pwstable.h pws_l1_path has the definition): ``motion`` (T, 4) float64 on the device as for ``smooth_path``,
    ``frame_hw`` = (H, W) of the frame whose pixels ``motion`` is in.  Per scene (``scene_cuts`` as for ``smooth_path``) the measured pose P
    = (log scale, angle, cx, cy) is ``smooth_path``'s, bit for bit; per component the path P^ inside the box |P^ - P| <= b minimises
    w1 |D1 P^|_1 + w2 |D2 P^|_1 + w3 |D3 P^|_1 (D_k: the k-th forward difference; the components in units of their b), so that it is made of
    static, constant-velocity and constant-acceleration pieces; D[k] = C_k^-1 o C^_k as for ``smooth_path``.  ``reach`` = c in (0, 0.5]
    is the share of the frame, per axis, that the path may move away from the measured one: b = (-log(1 - c), c min(H, W) / max(H, W),
    c W / 2, c H / 2).  Each half-width alone spends the whole share; together they are no coverage guarantee -- ``limit_path`` is.  The
    default 0.1, like the paper's weights (10, 1, 100), is a judgement that no footage here can fit.  The LP is solved on the device by a
    primal-dual interior-point method, at most 64 Newton steps; a scene of 3 frames or fewer keeps its path (D is the identity).
    Returns (D (T, 6), path (T, 4)) float64 on the device -- ``path`` is the MEASURED path -- [, info (scenes, 4, 4): per scene and
    component (Newton steps, the final gap s . l, the final scaled objective, converged 1 / 0)]; no synchronisation; three launches per
    scene, on slices, and one workspace allocation of 1 152 bytes per frame of the longest scene.  Fixed order: the same bits on every run.
    ValueError: a tensor that is not (T, 4) float64 on the device, reach outside (0, 0.5], weights that are not three positive finite
    numbers, bad cuts, a frame_hw that is not two integers >= 2, a scene above 65 536 frames."""
    _check_motion(motion, "optimal_path")
    reach, weights = _check_l1(reach, weights, "optimal_path")
    bound = _l1_bounds(reach, frame_hw, "optimal_path")
    motion = motion.contiguous()
    T = motion.shape[0]
    cuts = _cut_list(scene_cuts, T, "optimal_path")
    scenes = list(_scenes(T, cuts)) if T else []
    longest = max((b - a for a, b in scenes), default=0)
    if longest > 65536:
        raise ValueError("optimal_path: a scene of %d frames, at most 65536 (the solver's band solve is sequential)" % longest)
    d = torch.empty((T, 6), device=motion.device, dtype=torch.float64)
    path = torch.empty((T, 4), device=motion.device, dtype=torch.float64)
    info = torch.empty((len(scenes), 4, 4), device=motion.device, dtype=torch.float64)
    L = A.lib()
    nbytes = int(L.pws_l1_path_workspace(longest))
    ws = torch.empty((nbytes // 8,), device=motion.device, dtype=torch.float64)   # (stream-ordered: one scene after the other uses it)
    cb, cw = (ctypes.c_double * 4)(*bound), (ctypes.c_double * 3)(*weights)
    for i, (a, b) in enumerate(scenes):
        A.check(L.pws_l1_path(A.ptr(motion[a:b]), b - a, cb, cw, A.ptr(path[a:b]), A.ptr(d[a:b]), A.ptr(info[i]), A.ptr(ws), nbytes,
                              A.current_stream()), "pws_l1_path")
    return (d, path, info) if return_info else (d, path)


def shutter_rates(motion, scene_cuts=None):
    """The camera's velocity at every frame of a clip, for the rolling-shutter correction (csrc/path_smooth.hip; include/pwstable.h
    pws_shutter_rates has the definition): ``motion`` (T, 4) float64 on the device as for ``smooth_path``.  Returns (T, 2, 4) float64 on
    the device: per frame k the rates (log scale, angle, x, y per frame interval) in frame k's own coordinates, [k, 0] from the pair ahead
    (motion[k+1]), [k, 1] from the pair behind (motion[k]) -- what ``functional.compose_fields(rates=)`` takes.  Per scene
    (``scene_cuts`` as for ``smooth_path``): rates never cross a cut, a scene's first and last frame use their one pair twice, a scene of
    one frame has zero rates; a NaN row counts as no motion.  No synchronisation; one launch per scene, on slices; the same bits on every run.
    ValueError: a tensor that is not (T, 4) float64 on the device, bad cuts."""
    _check_motion(motion, "shutter_rates")
    motion = motion.contiguous()
    T = motion.shape[0]
    cuts = _cut_list(scene_cuts, T, "shutter_rates")
    rates = torch.empty((T, 2, 4), device=motion.device, dtype=torch.float64)
    for a, b in (_scenes(T, cuts) if T else []):
        A.check(A.lib().pws_shutter_rates(A.ptr(motion[a:b]), b - a, A.ptr(rates[a:b]), A.current_stream()), "pws_shutter_rates")
    return rates


def frame_sharpness(frames, pixel_format="bgr24", frames_are_rgb=False, out=None):
    """How sharp each frame is, for deblurring (csrc/deblur.hip; include/pwstable.h pws_frame_sharpness_u8 has the definition): ``frames`` in
    any integer ``pixel_format`` (``functional.keep_borders_``' shapes), on the device.  ``S[t]`` is the sum over the interior pixels of
    ``(I[y,x+1] - I[y,x-1])^2 + (I[y+1,x] - I[y-1,x])^2`` with the integer intensity I = ``(29 B + 150 G + 77 R + 128) >> 8`` for "bgr24"
    (``frames_are_rgb`` swaps the 29 and the 77), the Y plane for the packed YUV formats -- P010 / P210 words ``>> 6``, I010 / I210 / I410
    words clamped to 1023.  Measured on the frames themselves: on the 256 x 256 window planes a 5-tap blur shows as a ratio of 0.90, here as
    0.33.  Returns (T,) int64 on the device (``out``: a contiguous (T,) int64 device tensor to fill), no synchronisation.  Exact integer
    arithmetic: the same bits on every run.  ValueError: float frames, host tensors, a shape that does not fit, frames below 3 x 3."""
    if not isinstance(frames, torch.Tensor) or frames.dtype not in (torch.uint8, torch.uint16):
        raise ValueError("frame_sharpness: frames must be uint8 or uint16 (the integer pixel formats), got %s" % (getattr(frames, "dtype", type(frames)),))
    fmt = PF.lookup_format(pixel_format) or PF._packed_format(pixel_format, torch.uint8)   # (an unknown format is a ValueError)
    if fmt.hwc and (frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3):
        raise ValueError("frame_sharpness: bgr24 frames must be uint8 (T,H,W,3), got %s %s" % (frames.dtype, tuple(frames.shape)))
    n, h, w = fmt.frame_shape(frames)   # (packed frames: a tensor of the other depth's dtype is a ValueError)
    if h < 3 or w < 3:
        raise ValueError("frame_sharpness: frames must be at least 3 x 3 (the interior), got %d x %d" % (w, h))
    if not frames.is_cuda:
        raise ValueError("frame_sharpness: frames must be on the device (there is no CPU path)")
    if out is None:
        out = torch.empty((n,), device=frames.device, dtype=torch.int64)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != (n,) or not out.is_cuda or not out.is_contiguous():
        raise ValueError("frame_sharpness: out must be a contiguous (%d,) int64 tensor on the device" % n)
    frames = frames.contiguous()
    if fmt.hwc:
        A.check(A.lib().pws_frame_sharpness_u8(A.ptr(frames), n, h, w, int(bool(frames_are_rgb)), A.ptr(out), A.current_stream()), "pws_frame_sharpness_u8")
    elif fmt.dtype == torch.uint8:
        A.check(A.lib().pws_plane_sharpness_u8(A.ptr(frames), frames.shape[1] * w, n, h, w, A.ptr(out), A.current_stream()), "pws_plane_sharpness_u8")
    else:
        A.check(A.lib().pws_plane_sharpness_u16(A.ptr(frames), frames.shape[1] * w, n, h, w, fmt.layout, A.ptr(out), A.current_stream()),
                "pws_plane_sharpness_u16")
    return out


def deblur_plan(motion, sharpness, radius, scene_cuts=None):
    """Which neighbours lend a frame detail, and where (csrc/deblur.hip; include/pwstable.h pws_deblur_plan has the definition): ``motion``
    (T, 4) float64 on the device as ``global_motion(..., pixel_scale=(W / 256, H / 256))`` returns it -- row k maps frame k to frame k-1, in
    frame pixels about the frame centre -- ``sharpness`` (T,) int64 (``frame_sharpness``) and ``radius`` R in 1 .. 15.  Returns
    ``maps`` (T, 2R+1, 6) float64 -- ``maps[t, R+k]``, row-major 2 x 3, takes a centred position of frame t to frame t+k: the chain of the
    per-pair similarities, resp. of their inverses, walked outward from t; the centre column is the identity -- ``gain`` (T, 2R+1) float32,
    ``1 - S[t] / S[t+k]`` where frame t+k is sharper and 0 elsewhere, and ``donors`` (T,) int32, the positive gains per frame: what
    ``functional.deblur_frames`` takes.  A chain stops at the scene's ends (``scene_cuts`` as for ``smooth_path``) and at the first pair whose
    motion is not finite or whose scale lies outside [0.5, 2]: from there outward the map is NaN and the gain 0 -- a donor that is not
    aligned is worse than none.  On the device, no synchronisation; two launches per scene, on slices; the same bits on every run.
    One global similarity per pair: parallax and moving objects are not aligned, only down-weighted by ``deblur_frames``' sensitivity.
    ValueError: tensors other than these, on the device; a radius outside 1 .. 15; bad cuts."""
    _check_motion(motion, "deblur_plan")
    T = motion.shape[0]
    if (not isinstance(sharpness, torch.Tensor) or not sharpness.is_cuda or sharpness.dtype != torch.int64 or tuple(sharpness.shape) != (T,)):
        raise ValueError("deblur_plan: sharpness must be a (%d,) int64 tensor on the device" % T)
    radius, _ = PF._check_deblur(radius, 1.0, "deblur_plan")
    motion, sharpness = motion.contiguous(), sharpness.contiguous()
    cuts = _cut_list(scene_cuts, T, "deblur_plan")
    k = 2 * radius + 1
    maps = torch.empty((T, k, 6), device=motion.device, dtype=torch.float64)
    gain = torch.empty((T, k), device=motion.device, dtype=torch.float32)
    donors = torch.empty((T,), device=motion.device, dtype=torch.int32)
    for a, b in (_scenes(T, cuts) if T else []):
        A.check(A.lib().pws_deblur_plan(A.ptr(motion[a:b]), A.ptr(sharpness[a:b]), b - a, radius, A.ptr(maps[a:b]), A.ptr(gain[a:b]),
                                        A.ptr(donors[a:b]), A.current_stream()), "pws_deblur_plan")
    return maps, gain, donors


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
    _check_motion(motion, what)
    try:
        h, w = (int(v) for v in plane_hw)
    except (TypeError, ValueError):
        raise ValueError("%s: plane_hw must be (h, w), got %r" % (what, plane_hw)) from None
    radius = _check_radius(radius, h, w, what)
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
    cuts = _cut_list(scene_cuts, T, what)
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
    PF._field_operands("limit_path", fields, name="fields")
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
    cuts = _cut_list(scene_cuts, T, "limit_path")
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
    cuts = _cut_list(scene_cuts, T, "stability_scores")
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
