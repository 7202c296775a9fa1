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
import collections
import math
import time

import torch

from . import functional as PF
from .frameio import (_area_resize_yuv, _crop, _frames_shape, _output_resize, _window_planes, _yuv_crop, _yuv_format, _yuv_planes,  # noqa: F401
                      area_half, area_resize, area_resize_yuv, area_resize_yuv16, window_planes, window_planes_yuv, window_planes_yuv16)
from .framing import (_bounds_rows, _centred_window, _check_lattice, _field_homography, _has_lattice, auto_crop_window,  # noqa: F401
                      field_homography, zoom_schedule, zoom_window)
from .motion import (L1_REACH, L1_WEIGHTS, _check_l1, _check_limit, _check_max_se, _check_shutter, _check_sigma, block_motion, deblur_plan,  # noqa: F401
                     estimate_rolling_shutter, frame_sharpness, global_motion, limit_path, limit_rectangle, optimal_path, scene_scores,
                     shutter_rates, smooth_path, stability_scores)
from .scenes import _check_cuts, _cut_rule, _scenes, find_scene_cuts  # noqa: F401


def _check_integer_frames(frames, what, feature):
    """``feature`` -- borders="keep", borders="mosaic", an edge mode -- reads and writes integer samples; ValueError for other frames."""
    if frames.dtype not in (torch.uint8, torch.uint16):
        raise ValueError("%s: %s is for the integer pixel formats (uint8 / uint16 frames), got %s" % (what, feature, frames.dtype))


def _crop_window(fmt, oh, ow, crop):
    """(cy0, cy1, cx0, cx1): the window that ``crop`` = None or (x_start, x_end, y_start, y_end[, threshold]) cuts out of the oh x ow output
    frame in the format ``fmt``; ValueError for a window that does not lie inside it or, for packed frames, off the format's multiples."""
    cy0, cy1, cx0, cx1 = 0, oh, 0, ow
    if crop is not None:
        if len(crop) not in (4, 5):
            raise ValueError("crop must be (x_start, x_end, y_start, y_end[, threshold])")
        th = int(crop[4]) if len(crop) == 5 else 0
        cx0, cx1, cy0, cy1 = int(crop[0]) + th, int(crop[1]) - th, int(crop[2]) + th, int(crop[3]) - th
        if not (0 <= cx0 < cx1 <= ow and 0 <= cy0 < cy1 <= oh):
            raise ValueError("crop window x [%d, %d) y [%d, %d) does not lie inside the %d x %d output frame" % (cx0, cx1, cy0, cy1, ow, oh))
        mx, my = fmt.multiples if fmt.packed else (1, 1)
        if (cx0 | cx1) % mx or (cy0 | cy1) % my:
            if fmt.chroma == 0:
                raise ValueError("crop window x [%d, %d) y [%d, %d) of %s frames must have even edges" % (cx0, cx1, cy0, cy1, fmt.name))
            raise ValueError("crop window x [%d, %d) y [%d, %d) of %s frames must have edges that are multiples of %d (x) and %d (y)"
                             % (cx0, cx1, cy0, cy1, fmt.name, mx, my))
    return cy0, cy1, cx0, cx1


def _hand_over(warped, dest, lane, down):
    """``warped``, finished on the stream ``lane``, into ``dest``: host frames go down on the stream ``down`` behind one event; device frames
    (down None) are copied in place."""
    if down is None:
        dest.copy_(warped)
        return
    done = torch.cuda.Event()
    done.record(lane)
    with torch.cuda.stream(down):
        down.wait_event(done)
        dest.copy_(warped, non_blocking=True)
    warped.record_stream(down)


class StreamPlan(collections.namedtuple("StreamPlan", "fmt h w oh ow T n_all halo_left halo_right chunk chunks in_flight on_host half_size_output "
                                        "frames_are_rgb crop zmode zwin zoom_speed zoom_min two_pass mosaic radius keep rigid edge metrics lattice "
                                        "smooth shutter max_se wobble max_crop limit_levels limit_relax detect cuts scene_threshold scene_min_len deblur "
                                        "deblur_sensitivity path_model l1_reach l1_weights")):
    """Everything that run_video decides from its arguments and the stabiliser's options before it touches the device (VideoStabilizer._plan):
    the format record ``fmt``; the source ``h`` x ``w`` and the output ``oh`` x ``ow`` before the crop; the ``T`` frames to stabilise of the
    ``n_all`` given, the halos, ``chunk`` and the ``chunks`` [(start, stop)] in the index space of the frames (the first / last chunk carry
    the halo frames with them), ``in_flight`` lanes, ``on_host`` input; ``crop``: None, the window (cy0, cy1, cx0, cx1) of an explicit crop,
    or "auto"; ``zmode``: None, "fixed" (``zwin``, the one window), "auto" or "adaptive" (``zoom_speed``, ``zoom_min``); ``two_pass``: pass 1
    keeps fields and bounds, the host decides, pass 2 warps; ``mosaic`` and its ``radius``, ``keep``, ``rigid``, the ``edge`` mode,
    ``metrics``, ``lattice`` (the frame holds the homography fit's); ``smooth`` (sigma, 0: off), ``shutter`` (a float or "auto") and ``max_se``, ``wobble`` (sigma, 0: off), ``max_crop`` (None: off) with ``limit_levels`` and the resolved ``limit_relax``; ``detect``
    (scene_cuts="auto") with its thresholds, and ``cuts``, the checked list the call starts from; ``deblur`` (the radius, 0: off) and
    ``deblur_sensitivity``; ``path_model``: None (no smoothing), "gaussian" (``smooth`` is its sigma) or "l1" (``smooth`` is 0.0) with
    ``l1_reach`` and ``l1_weights``."""
    __slots__ = ()


def _prefetch(frames, s, e, stream, dev):
    """frames[s:e] on the device and the event to wait for: device-resident frames are read in place (no event), host frames go up on ``stream``."""
    if frames.is_cuda:
        return frames[s:e], None
    with torch.cuda.stream(stream):
        buf = frames[s:e].to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
    return buf, ev


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
                 limit_relax=None, shutter_max_se=0.02, deblur=0, deblur_sensitivity=4.0, l1_reach=L1_REACH, l1_weights=L1_WEIGHTS):
        self.net = netG
        # run_video lends every SOURCE frame detail from the sharper frames of its scene within `deblur` frames, 1 .. 15, aligned by the clip's
        # global motion, in front of the untouched warp (functional.deblur_frames; OpenCV videostab's order): shake blurs some frames and
        # leaves their neighbours sharp, and once the shake is gone the sharpness pulses.  deblur_sensitivity, in 8-bit gray levels: a donor
        # that far from the frame's own sample gets half its gain; 4.0 is a judgement that no footage here can fit, like zoom_speed.
        # 0: no launch, no allocation, every path as it was
        self.deblur, self.deblur_sensitivity = PF._check_deblur(deblur, deblur_sensitivity, "VideoStabilizer", zero_ok=True)
        self.deblur_sharpness = self.deblur_donors = None   # deblur > 0, of the last run_video, on the device: (T,) int64 / (T,) int32
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
        # smooth="l1": the path model is the L1-optimal path instead (optimal_path: static, constant-velocity and constant-acceleration pieces
        # inside a box of l1_reach of the frame per axis around the measured path, weights l1_weights on the three differences' L1 norms);
        # everything that needs smooth > 0 takes "l1" as smoothing on.  0.1 and the paper's (10, 1, 100) are judgements that no footage here
        # can fit, like zoom_speed
        self.smooth = "l1" if isinstance(smooth, str) and smooth == "l1" else _check_sigma(smooth, "VideoStabilizer", zero_ok=True)
        self.l1_reach, self.l1_weights = _check_l1(l1_reach, l1_weights, "VideoStabilizer")
        self.smooth_l1_info = None   # smooth="l1", of the last run_video, on the device: (scenes, 4, 4) float64, optimal_path's info
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
        # footage here can fit, like zoom_speed; under smooth="l1", which has no sigma, 1 / (period // 2): over the generator's own reach,
        # a judgement of the same kind.  None: no launch, no allocation, every path as it was
        self.max_crop, self.limit_levels, relax = _check_limit(max_crop, limit_levels, limit_relax, 0.0 if self.smooth == "l1" else self.smooth,
                                                               "VideoStabilizer")
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
    def run(self, gray, frames, halo_left=0, halo_right=0, out=None, pixel_format="bgr24", scene_cuts=None, keep_from=None, zoom=None):
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
        the device (no synchronisation).  Not with a zoom (ValueError).
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
        if mosaic:
            _check_integer_frames(frames, "run", "borders=\"mosaic\"")
        if keep:
            _check_integer_frames(frames, "run", "borders=\"keep\"")
        if self.edge != "pad":
            _check_integer_frames(frames, "run", "edge=%r" % (self.edge,))
        fmt = PF.frame_format(pixel_format, frames, "run", float_frames=True)   # (from here on the format is this record)
        if not (0 <= halo_left <= half and 0 <= halo_right <= half):
            raise ValueError("halo must be within [0, %d]" % half)
        T = frames.shape[0]
        if gray.shape[0] != T + halo_left + halo_right:
            raise ValueError("gray has %d frames, expected %d + %d + %d" % (gray.shape[0], T, halo_left, halo_right))
        cuts = _check_cuts(scene_cuts, gray.shape[0], "run") if scene_cuts is not None else None
        if zoom is not None or rigid:
            frame_hw = fmt.frame_shape(frames)[1:]
        if rigid:
            _check_lattice(int(frame_hw[0]), int(frame_hw[1]), "rigidity > 0")
        windows = PF._zoom_windows(zoom, T, frame_hw, "run") if zoom is not None else None
        # every check has passed: from here on the previous call's results go
        on_host = not frames.is_cuda
        dev = self.device
        self.mosaic_unfilled = torch.empty((T,), device=dev, dtype=torch.int32) if mosaic else None
        gray_d = gray.to(dev, non_blocking=True) if not gray.is_cuda else gray  # 256 KB per frame: copied once
        if out is None:
            out = torch.empty_like(frames, pin_memory=on_host) if on_host else torch.empty_like(frames)
        rres, runf = (torch.empty((T,), device=dev, dtype=torch.float32), torch.empty((T,), device=dev, dtype=torch.int32)) if rigid else (None, None)
        self.rigid_residual, self.rigid_unfit = rres, runf
        if zoom is not None:
            self.zoom_windows, self.zoom_uncovered = windows, torch.empty((T,), device=dev, dtype=torch.int32)
        if T == 0:
            return out
        copies = (torch.cuda.Stream(dev), torch.cuda.Stream(dev)) if on_host else (None, None)
        wall, fall = self._batches(fmt, gray_d, frames, halo_left, halo_right, cuts, out, copies, pad=0 if mosaic else None, keep_from=keep_from,
                                   zoom=(windows, self.zoom_uncovered) if zoom is not None else None, rigid_stats=(rres, runf))
        if mosaic:
            for a, b in _scenes(halo_left + T, cuts or (), halo_left):   # one scene piece per call: donors never cross a cut
                a, b = a - halo_left, b - halo_left
                PF.mosaic_borders_(wall[a:b], fall[a:b], self.mosaic_radius, pixel_format=pixel_format, align_corners=self.align_corners,
                                   mode=self.interpolation, _unfilled=self.mosaic_unfilled[a:b])
            _hand_over(wall, out, torch.cuda.current_stream(dev), copies[1])
            if on_host:
                copies[1].synchronize()
        return out

    def _warp(self, fmt, source, field, out=None):
        """One batch's warp -- the ``source`` frames by ``field``, into ``out`` if given -- and then the edge fill, if any: before a mosaic
        pass, where donors are read only where they are covered, so that exactly the unfilled positions show it."""
        source = source.contiguous()
        warped = PF.warp(source, field, fmt, swap_rb=self.swap_rb, align_corners=self.align_corners, out=out, mode=self.interpolation)
        if self.edge != "pad":
            PF.edge_borders_(warped, source, field, self.edge, fmt.name, swap_rb=self.swap_rb, align_corners=self.align_corners,
                             mode=self.interpolation)
        return warped

    def _batches(self, fmt, gray, frames, halo_left, halo_right, cuts, out, copies=(None, None), pad=None, keep_from=None, keep_wait=None,
                 zoom=None, rigid_stats=(None, None), hom_out=None):
        """The batch loop of run() and of run_video's single pass, arguments checked: ``gray`` on the device, ``frames`` (T > 0 of them) in the
        format ``fmt``, ``cuts`` a checked list in gray's index space or None.  Per batch: the generator, [the fit and the rigidity blend,]
        [the zoom,] the warp [and the edge fill], [the keep pass,] and frames s .. e-1 on their way to out[s:e].
        copies: the (upload, download) streams of host frames; the download stream has been waited for on return.
        keep_wait: the event behind the pass that wrote ``keep_from``, when another stream did (run_video's other lane).
        zoom = (windows, uncovered): the T checked windows and the (T,) counts to fill.
        rigid_stats = (residual, unfit) and hom_out = (M (T, 9), bounds (T, 4)): tensors of the T frames to fill -- run_video's, a slice
        per chunk, which it publishes itself once every chunk is issued; hom_out: the raw field's fit is kept (run_video(metrics=True)).
        pad (borders="mosaic"): nothing goes to ``out``.  The frames are warped with black borders into one buffer with ``pad`` spare frames at
        either end, and the fields that warped them are kept beside it, for the caller to fill.
        Returns (warped, fields): those two buffers, or (None, None) without ``pad``."""
        T, dev = frames.shape[0], self.device
        keep, rigid, mosaic = self.borders == "keep", self.rigidity > 0.0, pad is not None
        on_host = not frames.is_cuda
        h2d, d2h = copies
        rres, runf = rigid_stats
        if zoom is not None or rigid or hom_out is not None:
            frame_hw = fmt.frame_shape(frames)[1:]
        zcoef = None   # (the field's size is the generator's to say: formed at the first batch, uploaded once)
        gp, batches = self._layout(gray.contiguous(), halo_left, halo_right, T, cuts)
        compute = torch.cuda.current_stream(dev)
        nxt = _prefetch(frames, batches[0][0], batches[0][1], h2d, dev)
        pending = []
        cutset, prev = set(cuts or ()), None
        wall, fall = None, None   # borders="mosaic": the call's warped frames and fields
        for k, (s, e, start) in enumerate(batches):
            cur, ev = nxt
            if k + 1 < len(batches):
                nxt = _prefetch(frames, batches[k + 1][0], batches[k + 1][1], h2d, dev)  # overlaps with this batch's compute
            if ev is not None:
                compute.wait_event(ev)
            win = _windows(gp, start, e - s, self.period)
            field = self.net(win, False)
            if hom_out is not None or rigid:
                field = field.contiguous()
                if hom_out is not None:
                    hom, bounds = hom_out[0][s:e], hom_out[1][s:e]
                else:
                    hom, bounds = torch.empty((e - s, 9), device=dev, dtype=torch.float64), torch.empty((e - s, 4), device=dev, dtype=torch.float32)
                _field_homography(field, int(frame_hw[0]), int(frame_hw[1]), hom, bounds)
                if rigid:
                    field = PF._field_rigid(field, hom, frame_hw, self.rigidity, torch.empty_like(field), rres[s:e], runf[s:e])
            if zoom is not None:
                if zcoef is None:
                    zcoef = PF.zoom_coefficients(zoom[0], frame_hw, field.shape[1:3]).to(dev, non_blocking=True)
                field = field.contiguous()
                field = PF._field_zoom(field, zcoef[s:e], frame_hw, self.align_corners, self.interpolation, torch.empty_like(field), zoom[1][s:e])
            if mosaic:   # black borders into the call's buffer; the fill needs every batch
                if wall is None:
                    wall = torch.empty((T + 2 * pad,) + tuple(frames.shape[1:]), device=dev, dtype=frames.dtype)
                    fall = torch.empty((T + 2 * pad,) + tuple(field.shape[1:]), device=dev, dtype=torch.float32)
                self._warp(fmt, cur, field, wall[pad + s:pad + e])
                fall[pad + s:pad + e].copy_(field)
                if on_host:
                    cur.record_stream(compute)
                continue
            warped = self._warp(fmt, cur, field)
            if keep:
                if (s + halo_left) in cutset or (s == 0 and keep_from is None):
                    init, src = cur.contiguous()[0], True   # a scene's first frame: its own source, as the warp would write it
                elif prev is not None:
                    init, src = prev, False
                else:   # the caller's history: possibly written on another stream (run_video's other lane)
                    if keep_wait is not None:
                        compute.wait_event(keep_wait)
                    keep_from.record_stream(compute)
                    init, src = keep_from, False
                PF.keep_borders_(warped, field, init, fmt.name, initial_is_source=src, swap_rb=self.swap_rb, align_corners=self.align_corners,
                                 mode=self.interpolation)
                prev = warped[-1]   # (a view: keeps the batch alive until the next one has read it)
            _hand_over(warped, out[s:e], compute, d2h)
            if on_host:
                cur.record_stream(compute)
                pending.append(warped)
        if on_host and not mosaic:
            d2h.synchronize()
        return wall, fall

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
        VideoStabilizer(smooth="l1", l1_reach=0.1, l1_weights=(10.0, 1.0, 100.0)): the same route with the L1-optimal path (Grundmann, Kwatra,
        Essa, CVPR 2011; OpenCV videostab's LpMotionStabilizer) as the path model: ``optimal_path`` stands where ``smooth_path`` stands, on the
        same measured motion and cuts, and nothing else changes.  A Gaussian turns a hand-held "static" shot into a slow drift and bounds
        nothing; this path is exactly static, constant-velocity or constant-acceleration piece by piece, and it stays inside a box of
        l1_reach of the frame per axis around the measured path -- per component: the box is no coverage guarantee, max_crop stays that
        rule.  Everything that needs smooth > 0 takes "l1" as smoothing on: rolling_shutter, fixed and "auto", max_crop (limit_relax=None
        is 1 / (period // 2) here, the generator's own reach: a judgement), the halo and borders errors.  ``self.smooth_l1_info`` (scenes,
        4, 4) float64 -- per scene and component: Newton steps, final gap, final objective, converged -- is left on the device; None
        otherwise.  Reach and weights are judgements that no footage here can fit; similarity motion measured on the 256 x 256 planes, as
        before.  ValueError: l1_reach outside (0, 0.5], l1_weights that are not three positive finite numbers, a scene above 65 536 frames.
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
        VideoStabilizer(deblur=R, deblur_sensitivity=4.0), R in 1 .. 15 frames: deblurring (OpenCV videostab's ``WeightingDeblurer``).  Shake
        blurs some frames and leaves their neighbours sharp; once the shake is gone the sharpness pulses.  Every SOURCE frame borrows detail
        from the sharper frames of its scene within R frames, in front of the untouched warp.  The call takes the two-pass route, also
        without a crop, zoom, smooth or wobble.  Pass 1: the upload stream also computes ``frame_sharpness`` of each uploaded chunk, beside
        its window planes.  Between the passes, on the caller's stream: ``global_motion(input planes, pixel_scale=(W / 256, H / 256))`` --
        the INPUT's own motion, whatever the fields do -- then ``deblur_plan`` under the call's cuts.  Pass 2 prefetches frames
        [s - R, e + R) of each chunk, clipped to the clip (host frames are uploaded again with the overlap, device frames are read in place),
        deblurs the chunk into a buffer of its own (``functional.deblur_frames``: every read is of the original frames, so chunks give the
        bytes of one call over the clip), and everything behind reads that buffer as its source: zoom, warp, edge pass, metrics planes,
        resize and crop.  Packed YUV frames have their luma deblurred and their chroma left alone.  Left on the device, no synchronisation,
        None at deblur = 0, which takes no new path: ``self.deblur_sharpness`` (T,) int64 -- of the SOURCE frames -- and ``self.deblur_donors``
        (T,) int32, the neighbours each frame borrowed from.  One global similarity per pair: parallax and moving objects are guarded by the
        sensitivity term alone; sensor noise raises every frame's sharpness alike and shrinks the gains; nothing was validated on real
        footage.  Every integer pixel_format, interpolation, edge, crop, zoom, rigidity, wobble, smooth, max_crop, scene_cuts (also "auto"),
        in_flight and metrics works as without it.  ValueError: halos, borders="keep" or "mosaic" (no second pass), float frames, R outside
        0 .. 15, a sensitivity that is not finite and positive.  ``run()`` does not take it.
        Returns (T, H, W, 3) -- or (T, H/2, W/2, 3) / (T, height, width, 3), or the crop window of it -- uint8 on the inputs' side; for YUV
        (T, oh * 3 // 2, ow) of the output (or crop window) size oh x ow."""
        plan = self._plan(frames, chunk, half_size_output, frames_are_rgb, halo_left, halo_right, crop, output_size, in_flight, pixel_format,
                          scene_cuts, scene_threshold, scene_min_len, zoom, zoom_speed, zoom_min, metrics)
        self._reset(plan)
        call = _Call(self, plan, frames)
        if plan.T == 0:
            return call.out
        call.open()   # buffers and lanes
        try:
            for c in range(len(plan.chunks)):
                call.chunk(c)   # pass 1, or the single pass
            call.drain()
        finally:
            call.join()
        call.publish()
        if plan.two_pass:
            call.between_passes()
            call.pass2()
        if plan.metrics:
            call.measure()
        if plan.on_host:
            call.down.synchronize()
        return call.out

    def _plan(self, frames, chunk=32, half_size_output=False, frames_are_rgb=False, halo_left=0, halo_right=0, crop=None, output_size=None,
              in_flight=1, pixel_format="bgr24", scene_cuts=None, scene_threshold=0.25, scene_min_len=16, zoom=None, zoom_speed=0.002,
              zoom_min=0.5, metrics=None):
        """run_video's arguments and this object's options resolved into a StreamPlan, or the ValueError they deserve: every check that
        needs no data from the device, in one fixed order (when two rules are violated the earlier one speaks).  Host arithmetic on
        ``frames``' shape, dtype and side only: no device call, no allocation, nothing of ``self`` changes, and a CPU or "meta" tensor
        will do.  What depends on the clip -- the automatic crop, the zoom windows, an empty even window -- is run_video's to raise."""
        half = self.period // 2
        if not (0 <= halo_left <= half and 0 <= halo_right <= half):
            raise ValueError("halo must be within [0, %d]" % half)
        n_all = frames.shape[0]
        T = n_all - halo_left - halo_right
        if T < 0:
            raise ValueError("frames holds %d frames, fewer than the halos %d + %d" % (n_all, halo_left, halo_right))
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
        halos = bool(halo_left or halo_right)
        second_pass = self.borders not in ("keep", "mosaic")   # (they finish every frame in the single pass)
        auto = isinstance(crop, str)
        if auto:
            if crop != "auto":
                raise ValueError("crop must be None, \"auto\" or (x_start, x_end, y_start, y_end[, threshold])")
            if halos:
                raise ValueError("run_video: crop=\"auto\" needs the whole clip (a shard cannot see the clip's crop recurrence): gather "
                                 "the shards' field_homography bounds and pass crop=auto_crop_window(...)")
            if not second_pass:
                raise ValueError("run_video: crop=\"auto\" removes the wedges that borders=\"%s\" fills: choose one" % self.borders)
            _check_lattice(h, w)
        metrics = self.metrics if metrics is None else bool(metrics)
        if self.edge != "pad":
            _check_integer_frames(frames, "run_video", "edge=%r" % (self.edge,))
        mosaic, radius = self.borders == "mosaic", self.mosaic_radius
        if mosaic:
            _check_integer_frames(frames, "run_video", "borders=\"mosaic\"")
            if max(1, int(in_flight)) > 1:
                raise ValueError("run_video: borders=\"mosaic\" finishes a chunk one chunk late, which across two lanes needs an event design of "
                                 "its own: use in_flight=1")
            if int(chunk) < radius:
                raise ValueError("run_video: chunk=%d is shorter than mosaic_radius=%d: a chunk's donors must lie in the adjacent chunks" % (chunk, radius))
        rigid = self.rigidity > 0.0
        if rigid:
            _check_lattice(h, w, "rigidity > 0")
        zmode = zwin = None
        if zoom is not None:
            if crop is not None:
                raise ValueError("run_video: zoom fills the frame that a crop would cut: give zoom or crop, not both")
            if not second_pass:
                raise ValueError("run_video: zoom removes the wedges that borders=\"%s\" fills: choose one" % self.borders)
            if isinstance(zoom, str):
                if zoom not in ("auto", "adaptive"):
                    raise ValueError("zoom must be None, a fraction in (0, 1], \"auto\" or \"adaptive\", got %r" % (zoom,))
                if halos:
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
        path_model = "l1" if self.smooth == "l1" else "gaussian" if self.smooth > 0.0 else None
        smoothing, sigma = path_model is not None, 0.0 if path_model == "l1" else self.smooth
        l1_reach, l1_weights = _check_l1(self.l1_reach, self.l1_weights, "run_video")   # (the attributes can be set after construction)
        rs = _check_shutter(self.rolling_shutter, "run_video")   # (the attributes can be set after construction)
        max_se = _check_max_se(self.shutter_max_se, "run_video")
        if rs != 0.0 and not smoothing:
            raise ValueError("run_video: rolling_shutter=%r needs smooth > 0" % (self.rolling_shutter,))
        relax = 1.0 / max(1, half) if path_model == "l1" and self.limit_relax is None else self.limit_relax   # (no sigma: the generator's reach)
        max_crop, limit_levels, limit_relax = _check_limit(self.max_crop, self.limit_levels, relax, sigma, "run_video")
        if max_crop is not None and not smoothing:   # (the attributes can be set after construction)
            raise ValueError("run_video: max_crop=%r needs smooth > 0" % (self.max_crop,))
        if smoothing:
            if halos:
                raise ValueError("run_video: smooth > 0 needs the whole clip (a shard cannot see the scene's path)")
            if not second_pass:
                raise ValueError("run_video: smooth > 0 warps in a second pass, which borders=\"%s\" does not have yet" % self.borders)
        wob = PF._check_wobble(self.wobble, "run_video", zero_ok=True)   # (the attribute can be set after construction)
        if wob > 0.0:
            if halos:
                raise ValueError("run_video: wobble > 0 needs the whole clip (a shard cannot see its neighbours' fields)")
            if not second_pass:
                raise ValueError("run_video: wobble > 0 warps in a second pass, which borders=\"%s\" does not have yet" % self.borders)
            _check_lattice(h, w, "wobble > 0")
        deblur, dsens = PF._check_deblur(self.deblur, self.deblur_sensitivity, "run_video", zero_ok=True)   # (the attributes can be set after construction)
        if deblur > 0:
            if halos:
                raise ValueError("run_video: deblur > 0 needs the whole clip (a shard cannot see its neighbours' sharpness or the scene's motion)")
            if not second_pass:
                raise ValueError("run_video: deblur > 0 reads the source in a second pass, which borders=\"%s\" does not have yet" % self.borders)
            _check_integer_frames(frames, "run_video", "deblur=%d" % deblur)
        # pass 1: fields and bounds; the host's decision; pass 2: the warp
        two_pass = auto or zmode in ("auto", "adaptive") or smoothing or wob > 0.0 or deblur > 0
        detect = isinstance(scene_cuts, str)
        if detect and scene_cuts != "auto":
            raise ValueError("scene_cuts must be None, \"auto\" or a sorted sequence of frame indices, got %r" % (scene_cuts,))
        cuts = () if detect or scene_cuts is None else tuple(_check_cuts(scene_cuts, n_all, "run_video"))
        window = crop if auto or crop is None else _crop_window(fmt, oh, ow, crop)
        # chunk bounds in the index space of `frames`: the first / last chunk carry the halo frames with them.  (An empty clip has none, and
        # returns before anything reads ``chunk`` or ``in_flight``: whatever they hold is no error there, as it never was)
        chunks = tuple((s if s > halo_left else 0, min(halo_left + T, s + chunk) if s + chunk < halo_left + T else n_all)
                       for s in range(halo_left, halo_left + T, chunk)) if T > 0 else ()
        return StreamPlan(fmt, h, w, oh, ow, T, n_all, halo_left, halo_right, chunk, chunks, max(1, int(in_flight)) if T > 0 else 1, not frames.is_cuda,
                          bool(half_size_output), bool(frames_are_rgb), window, zmode, zwin, zoom_speed, zoom_min, bool(two_pass), mosaic, radius,
                          self.borders == "keep", rigid, self.edge, metrics, _has_lattice(h, w), sigma, rs, max_se, wob, max_crop, limit_levels,
                          limit_relax, detect, cuts, scene_threshold, scene_min_len, deblur, dsens, path_model, l1_reach, l1_weights)

    def _reset(self, plan):
        """What the previous run_video left goes, in one place, once the plan stands: every result is None until this call sets it."""
        self.zoom_windows = self.zoom_uncovered = None
        self.rigid_residual = self.rigid_unfit = None
        self.mosaic_unfilled = None
        self.motion_in = self.motion_out = self.motion_inliers_in = self.motion_inliers_out = self._report = None
        self.smooth_motion = self.smooth_inliers = self.smooth_path = self.smooth_correction = self.smooth_uncovered = None
        self.smooth_l1_info = None
        self.shutter_rates = self.shutter_estimate = self.rolling_shutter_used = None
        self.limit_strength = self.limit_need = self.limit_uncovered = self.smooth_correction_unlimited = None
        self.wobble_removed = self.wobble_unfit = None
        self.deblur_sharpness = self.deblur_donors = None
        self.scene_cuts = list(plan.cuts)   # scene_cuts="auto" extends it chunk by chunk
        if plan.detect:
            self.scene_wait_s = 0.0   # host time spent waiting for scores (tools/scene_cuts_bench.py)

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


class _Call:
    """One run_video call in flight: the plan, the streams and lanes, the clip's buffers, and what one step leaves for the next -- the staged
    uploads, the cut detection's scores, the mosaic's waiting chunk, the keep pass's last frame.  run_video names the steps in their order."""

    def __init__(self, vs, plan, frames):
        self.vs, self.plan, self.frames = vs, plan, frames
        self.cuts = vs.scene_cuts   # (the one list: what detection appends, the stabiliser shows)
        self.cropping = plan.crop is not None
        self.window = plan.crop if isinstance(plan.crop, tuple) else (0, plan.oh, 0, plan.ow)   # (cy0, cy1, cx0, cx1); "auto": after pass 1
        self.out = None if plan.crop == "auto" and plan.T > 0 else self.alloc_out()

    def alloc_out(self):
        p = self.plan
        cy0, cy1, cx0, cx1 = self.window
        oshape = _frames_shape(p.fmt, p.T, cy1 - cy0, cx1 - cx0)
        if p.on_host:
            return torch.empty(oshape, dtype=self.frames.dtype, pin_memory=True)
        return torch.empty(oshape, dtype=self.frames.dtype, device=self.vs.device)

    def open(self):
        """The streams, the lanes and every buffer that lives as long as the call."""
        vs, p, dev = self.vs, self.plan, self.vs.device
        T = p.T
        self.compute = compute = torch.cuda.current_stream(dev)
        self.up, self.down = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        self.rres = self.runf = None
        if p.rigid:   # (before the lanes fork from the caller's stream: every lane writes its chunks' slices)
            self.rres = torch.empty((T,), device=dev, dtype=torch.float32)
            self.runf = torch.empty((T,), device=dev, dtype=torch.int32)
        self.mhom = self.mbounds = None
        if p.metrics:   # (also before the fork) the output planes; below the fit's lattice size cropping and distortion are not reported
            self.planes_out = torch.empty((T, 256, 256), device=dev, dtype=torch.float32)
            self.out_rgb = (p.frames_are_rgb != vs.swap_rb) if not p.fmt.packed else False   # the warp's swap_rb turns the channel order round
            if p.lattice and not p.two_pass:   # (the two-pass paths keep their own fit)
                self.mhom = torch.empty((T, 9), device=dev, dtype=torch.float64)
                self.mbounds = torch.empty((T, 4), device=dev, dtype=torch.float32)
        # (the lanes live as long as the stabiliser: the generator keeps an arena / a graph per STREAM, and torch's allocator a pool per stream)
        # The caller's stream is lane 0: the runtime deals streams to a handful of hardware queues, and a lane that shares its queue with
        # the upload or the download stream waits behind their copies (two NEW lanes beside up / down: 1 744 -> 1 291 frames/s).
        while len(vs._lanes) < p.in_flight - 1:
            vs._lanes.append(torch.cuda.Stream(dev))
        self.lanes = [compute] + vs._lanes[:p.in_flight - 1]
        self.mod = mod = getattr(vs.net, "module", vs.net)
        self.restore = None
        if p.in_flight > 1:
            self.restore = (mod._graph_mode, mod._graph_alias, getattr(mod, "_graph_per_stream", False), mod.two_queues)
            mod.two_queues = False   # two forwards that both fork into the device's one side queue would serialise there
            if mod._graph_mode:
                mod.enable_graph(True, mod._graph_alias, per_stream=True)
            for lane in self.lanes[1:]:
                lane.wait_stream(compute)
        self.gray_all = torch.empty((p.n_all, 256, 256), device=dev, dtype=torch.float32)
        if p.zmode is not None:
            self.zunc = torch.empty((T,), device=dev, dtype=torch.int32)
        if p.two_pass:
            self.fields = torch.empty((T, 256, 256, 2), device=dev, dtype=torch.float32)
            self.hom = torch.empty((T, 9), device=dev, dtype=torch.float64)
            self.bounds = torch.empty((T, 4), device=dev, dtype=torch.float32)
        if p.deblur > 0:   # (no halos: the frames given are the T core frames)
            self.sharp = torch.empty((T,), device=dev, dtype=torch.int64)
        self.up.wait_stream(compute)   # gray_all was allocated on the compute stream
        self.pend = None   # borders="mosaic": the chunk that waits for its successor -- (warped, fields, cs, ce, buf, valid frames of the head pad)
        if p.mosaic:
            self.unf = torch.empty((T,), device=dev, dtype=torch.int32)
        self.staged, self.uploaded = {}, 0
        self.carry, self.carried = None, None   # borders="keep": the last warped (pre-resize) frame so far, and the event behind the pass that made it
        if p.detect:
            self.scores_h = torch.empty((p.n_all,), dtype=torch.float32, pin_memory=True)
            self.scored, self.decided = {}, 0

    def upload(self, c):
        p = self.plan
        s, e = p.chunks[c]
        with torch.cuda.stream(self.up):
            buf = self.frames[s:e].to(self.vs.device, non_blocking=True) if p.on_host else self.frames[s:e]
            _window_planes(buf, p.fmt, 256, self.gray_all[s:e], "run_video", p.frames_are_rgb)
            if p.deblur > 0:   # beside the planes, from the same uploaded frames
                frame_sharpness(buf, p.fmt.name, p.frames_are_rgb, out=self.sharp[s:e])
            ev = torch.cuda.Event()
            ev.record(self.up)
            if p.detect:   # same stream: ordered behind the planes (and behind the previous chunk's, whose last plane it reads)
                s0 = max(s - 1, 0)
                self.scores_h[s:e].copy_(scene_scores(self.gray_all[s0:e])[s - s0:], non_blocking=True)
                self.scored[c] = torch.cuda.Event()
                self.scored[c].record(self.up)
        return buf, ev

    def detect_cuts(self, need):
        """extends the cut list over the planes 0 .. need-1 (the host waits for the upload that scored plane need-1)"""
        p = self.plan
        k = next(k for k, (s, e) in enumerate(p.chunks) if e >= need)
        t0 = time.perf_counter()
        self.scored[k].synchronize()
        self.vs.scene_wait_s += time.perf_counter() - t0
        first = max(self.decided, 1)
        self.cuts.extend(_cut_rule(self.scores_h[first:need].tolist(), first, self.cuts[-1] if self.cuts else 0, p.scene_threshold, p.scene_min_len))
        self.decided = max(self.decided, need)

    def chunk(self, c):
        """Chunk c on its lane: the uploads it needs, its cuts, and pass 1 or the single pass."""
        vs, p = self.vs, self.plan
        half = vs.period // 2
        s, e = p.chunks[c]
        lane = self.lanes[c % len(self.lanes)]
        # a chunk's windows reach `half` frames past its end: every chunk that holds one of those frames must be on the
        # device (and its planes computed) first; one chunk further ahead keeps the upload stream busy during this compute
        need = min(p.n_all, e + half)
        while self.uploaded < len(p.chunks) and (p.chunks[self.uploaded][0] < need or self.uploaded <= c + 1):
            self.staged[self.uploaded] = self.upload(self.uploaded)
            self.uploaded += 1
        for k in range(c, self.uploaded):
            if p.chunks[k][0] < need:
                lane.wait_event(self.staged[k][1])
        # (planes of EARLIER chunks that this one's windows reach back into were produced before staged[c]'s event on the same stream)
        buf, ev = self.staged.pop(c)
        # core frames of this chunk (the halo frames at the clip's ends are uploaded with it but not stabilised)
        cs, ce = max(s, p.halo_left), min(e, p.halo_left + p.T)
        hl, hr = min(half, cs), min(half, p.n_all - ce)
        if p.detect:
            self.detect_cuts(ce + hr)
        # the cuts inside this chunk's slice of the planes, in the slice's index space (None without cuts: the path as it was)
        sc = [t - (cs - hl) for t in self.cuts if cs - hl < t < ce + hr] or None
        gray = self.gray_all[cs - hl:ce + hr]
        with torch.cuda.stream(lane):
            if p.two_pass:
                self.pass1(gray, hl, hr, cs, ce, sc)
            else:
                self.single_pass(gray, hl, hr, cs, ce, sc, buf, s, lane)

    def pass1(self, gray, hl, hr, cs, ce, sc):
        """fields and per-frame bounds only (no halos here: core frames = output positions)"""
        vs, p = self.vs, self.plan
        fields, hom = self.fields[cs:ce], self.hom[cs:ce]
        vs._fields(gray, hl, hr, fields, sc)
        if (p.path_model is None or p.rigid or p.wobble > 0.0) and p.lattice:   # (smoothing fits the fields it composes, between the passes; the
            # blend and the wobble filter need the raw fit; deblurring alone takes the two passes at any size and needs no fit)
            _field_homography(fields, p.h, p.w, hom, self.bounds[cs:ce])
        if p.rigid:   # the kept fields, in place; the bounds stay the raw fit's
            PF._field_rigid(fields, hom, (p.h, p.w), vs.rigidity, fields, self.rres[cs:ce], self.runf[cs:ce])

    def single_pass(self, gray, hl, hr, cs, ce, sc, buf, s, lane):
        """the chunk's core frames buf[cs - s:ce - s] through the batch loop and on to ``out``"""
        vs, p = self.vs, self.plan
        a, b = cs - p.halo_left, ce - p.halo_left   # (output positions)
        core = buf[cs - s:ce - s]
        fill = {"rigid_stats": (self.rres[a:b], self.runf[a:b]) if p.rigid else (None, None),
                "hom_out": (self.mhom[a:b], self.mbounds[a:b]) if self.mhom is not None else None}
        if p.mosaic:   # warped with black borders; the chunk before it is filled and finished
            wall, fall = vs._batches(p.fmt, gray, core, hl, hr, sc, None, pad=p.radius, **fill)
            self.mosaic_step((wall, fall, cs, ce, buf), lane)
            return
        warped = torch.empty_like(core)
        # ("fixed": the one window, in the single pass)
        zoom = (PF._zoom_windows(p.zwin, ce - cs, (p.h, p.w), "run"), self.zunc[a:b]) if p.zmode is not None else None
        vs._batches(p.fmt, gray, core, hl, hr, sc, warped, zoom=zoom, keep_from=self.carry, keep_wait=self.carried, **fill)
        if p.keep:   # the next chunk's pass (on the other lane, if any) starts from this chunk's last frame: no copy, one event
            self.carry = warped[-1]
            if len(self.lanes) > 1:
                self.carried = torch.cuda.Event()
                self.carried.record(lane)
        self.finish(warped, buf, a, b, lane)

    def finish(self, warped, buf, s, e, lane):
        """output resize + crop of the warped core frames s .. e-1 (output positions) on `lane`, and their way to `out`"""
        p = self.plan
        if p.metrics:   # the planes of what the viewer sees, at the warp's size
            _window_planes(warped, p.fmt, 256, self.planes_out[s:e], "run_video", self.out_rgb)
        if (p.oh, p.ow) != (p.h, p.w):
            warped = _output_resize(warped, p.fmt, (p.ow, p.oh), p.half_size_output)
        if self.cropping:
            warped = _crop(warped, p.fmt, p.oh, p.ow, *self.window)
        if p.on_host:
            buf.record_stream(lane)
        _hand_over(warped, self.out[s:e], lane, self.down if p.on_host else None)

    def mosaic_step(self, new, lane):
        """chunk `new` = (warped, fields, cs, ce, buf), both buffers with `radius` spare frames at either end, has been warped (None: the
        clip is over): the waiting chunk takes its first frames as donors, is filled scene by scene and finished; `new` takes the
        waiting chunk's last frames and waits in its turn.  (Filled frames are as good donors as the warp's own.)"""
        vs, p = self.vs, self.plan
        R, pend = p.radius, self.pend
        if pend is not None:
            pw, pf, ps, pe, pbuf, nt = pend
            nh = 0
            if new is not None:
                nh = min(R, new[3] - new[2])
                pw[R + pe - ps:R + pe - ps + nh].copy_(new[0][R:R + nh])
                pf[R + pe - ps:R + pe - ps + nh].copy_(new[1][R:R + nh])
            lo, hi, off = ps - nt, pe + nh, R - ps   # the frames the buffer holds (index space of `frames`); frame g is at g + off
            for a, b in _scenes(p.halo_left + p.T, self.cuts, p.halo_left):
                fa, fb = max(a, ps), min(b, pe)
                if fa < fb:
                    da, db = max(a, lo), min(b, hi)
                    PF.mosaic_borders_(pw[da + off:db + off], pf[da + off:db + off], R, fa - da, fb - da, pixel_format=p.fmt.name,
                                       align_corners=vs.align_corners, mode=vs.interpolation, _unfilled=self.unf[fa - p.halo_left:fb - p.halo_left])
            self.finish(pw[R:R + pe - ps], pbuf, ps - p.halo_left, pe - p.halo_left, lane)
        if new is not None:
            nt = 0
            if pend is not None:
                nt = min(R, pe - ps)
                new[0][R - nt:R].copy_(pw[R + pe - ps - nt:R + pe - ps])
                new[1][R - nt:R].copy_(pf[R + pe - ps - nt:R + pe - ps])
            self.pend = tuple(new) + (nt,)
        else:
            self.pend = None

    def drain(self):
        """Every chunk is issued: borders="mosaic" finishes the last one."""
        if self.plan.mosaic:
            self.mosaic_step(None, self.compute)
            self.vs.mosaic_unfilled = self.unf

    def join(self):
        """The lanes join the caller's stream and the generator gets its settings back, whatever happened."""
        if self.restore is not None:
            for lane in self.lanes[1:]:
                self.compute.wait_stream(lane)   # the caller's stream sees every chunk; gray_all and the outputs may be freed behind it
            self.mod.two_queues = self.restore[3]
            self.mod.enable_graph(self.restore[0], self.restore[1], per_stream=self.restore[2])

    def publish(self):
        """The per-frame results that the chunks filled slice by slice."""
        vs, p = self.vs, self.plan
        if p.rigid:
            vs.rigid_residual, vs.rigid_unfit = self.rres, self.runf
        if p.zmode is not None:
            vs.zoom_windows, vs.zoom_uncovered = [p.zwin] * p.T if p.zmode == "fixed" else None, self.zunc

    def between_passes(self):
        """Every lane has joined the caller's stream: the kept fields (after rigidity) are complete, and so is the cut list.  On that stream,
        in this order: the deblurring plan (from the input's planes and sharpness alone), wobble, the measurement, the "auto" shutter estimate and its one host read, smooth_path, shutter_rates, limit_path,
        the composition and refit per chunk, the zoom windows, the automatic crop and the output's allocation."""
        vs, p, dev = self.vs, self.plan, self.vs.device
        h, w, T = p.h, p.w, p.T
        cuts = self.cuts or None
        rs = p.shutter
        if p.deblur > 0:   # the INPUT's own motion, in frame pixels: deblurring acts on the source frames, whatever the fields do with them
            vs.deblur_sharpness = self.sharp
            dmotion, _ = global_motion(self.gray_all, pixel_scale=(w / 256.0, h / 256.0))
            self.dmaps, self.dgain, vs.deblur_donors = deblur_plan(dmotion, self.sharp, p.deblur, scene_cuts=cuts)
            del dmotion
        if p.wobble > 0.0:
            self.fields, vs.wobble_removed, vs.wobble_unfit = PF.wobble_fields(self.fields, self.hom, (h, w), p.wobble, scene_cuts=cuts, return_stats=True)
            if p.path_model is None:   # bounds, crop and zoom decisions and the report describe the field that warps (smoothing fits what it composes)
                _field_homography(self.fields, h, w, self.hom, self.bounds)
        fields = self.fields
        if p.path_model is not None:   # ... and it measures the filtered fields
            scale = (w / 256.0, h / 256.0)   # frame pixels per plane pixel
            seen = PF.grid_sample(self.gray_all.unsqueeze(1), fields, align_corners=vs.align_corners).squeeze(1)   # the planes as the fields warp them
            if rs == "auto":   # the blocks behind the fit are kept for the estimate: the same launches, the same motion
                vs.smooth_motion, vs.smooth_inliers, mv, sad, act = global_motion(seen, pixel_scale=scale, return_blocks=True)
                vs.shutter_estimate = estimate_rolling_shutter(vs.smooth_motion, mv, sad, act, tuple(seen.shape[1:]), pixel_scale=scale,
                                                               scene_cuts=cuts, frame_height=h)
                del mv, sad, act
                r_hat, se = vs.shutter_estimate.tolist()[:2]   # the one read of "auto": 32 bytes, and the host waits for pass 1 here
                rs = min(1.0, max(-1.0, r_hat)) if math.isfinite(r_hat) and se <= p.max_se else 0.0
                vs.rolling_shutter_used = rs
            else:
                vs.smooth_motion, vs.smooth_inliers = global_motion(seen, pixel_scale=scale)
            del seen
            if p.path_model == "l1":
                vs.smooth_correction, vs.smooth_path, vs.smooth_l1_info = optimal_path(vs.smooth_motion, (h, w), p.l1_reach, p.l1_weights,
                                                                                       scene_cuts=cuts, return_info=True)
            else:
                vs.smooth_correction, vs.smooth_path = smooth_path(vs.smooth_motion, p.smooth, scene_cuts=cuts)
            vs.smooth_uncovered = torch.empty((T,), device=dev, dtype=torch.int32)
            if rs != 0.0:   # the velocity at every frame, from the same measured motion and under the same cuts
                vs.shutter_rates = shutter_rates(vs.smooth_motion, scene_cuts=cuts)
            if p.max_crop is not None:   # the crop budget: every frame's share of its correction, decided on the kept fields, read in place
                vs.smooth_correction_unlimited = vs.smooth_correction
                vs.smooth_correction, vs.limit_strength, vs.limit_need, vs.limit_uncovered = limit_path(
                    vs.smooth_correction, fields, (h, w), 1.0 - p.max_crop, levels=p.limit_levels, relax=p.limit_relax, scene_cuts=cuts,
                    rates=vs.shutter_rates, rolling_shutter=rs, align_corners=vs.align_corners, mode=vs.interpolation)
            scratch = torch.empty((min(int(p.chunk), T),) + tuple(fields.shape[1:]), device=dev, dtype=torch.float32)
            for s in range(0, T, scratch.shape[0]):
                e = min(T, s + scratch.shape[0])
                if rs != 0.0:
                    PF._field_compose_rows(fields[s:e], vs.smooth_correction[s:e], vs.shutter_rates[s:e], rs, (h, w), vs.align_corners,
                                           vs.interpolation, scratch[:e - s], vs.smooth_uncovered[s:e])
                else:
                    PF._field_compose(fields[s:e], vs.smooth_correction[s:e], (h, w), vs.align_corners, vs.interpolation, scratch[:e - s],
                                      vs.smooth_uncovered[s:e])
                fields[s:e].copy_(scratch[:e - s])
                if p.lattice:   # bounds, crop and zoom decisions and the report describe the field that warps
                    _field_homography(fields[s:e], h, w, self.hom[s:e], self.bounds[s:e])
            del scratch
        if p.zmode == "auto":   # (the copy of the bounds to the host waits for pass 1)
            vs.zoom_windows = [zoom_window(auto_crop_window(self.bounds, (h, w), None, vs.period, scene_cuts=cuts), (h, w))] * T
        elif p.zmode == "adaptive":
            vs.zoom_windows = zoom_schedule(self.bounds, (h, w), p.zoom_speed, p.zoom_min, scene_cuts=cuts)
        if p.zmode is not None:   # (a fixed fraction under smoothing: its one window, in pass 2)
            self.zcoef = PF.zoom_coefficients(PF._zoom_windows(vs.zoom_windows, T, (h, w), "run_video"), (h, w), fields.shape[1:3]).to(dev, non_blocking=True)
        if p.crop == "auto":
            crop = auto_crop_window(self.bounds, (h, w), (p.oh, p.ow), vs.period, scene_cuts=cuts)   # (the copy to the host waits for pass 1)
            if p.fmt.packed:   # the BGR path's window, rounded inward to the format's multiples (4:2:0: even edges; 4:4:4: as it is)
                mx, my = p.fmt.multiples
                x0, x1, y0, y1 = int(crop[0]), int(crop[1]), int(crop[2]), int(crop[3])
                crop = (x0 + (-x0) % mx, x1 - x1 % mx, y0 + (-y0) % my, y1 - y1 % my)
                if not (crop[1] > crop[0] and crop[3] > crop[2]):
                    raise ValueError("run_video: the even crop window x [%d, %d) y [%d, %d) is empty" % crop)
            self.window = _crop_window(p.fmt, p.oh, p.ow, crop)
            self.out = self.alloc_out()

    def pass2(self):
        """[deblur +] [zoom +] warp + output resize + crop with the kept fields; chunk k+1 uploads while chunk k computes"""
        vs, p = self.vs, self.plan
        R = p.deblur   # deblurring reads frames [s - R, e + R) of each chunk, clipped to the clip: host frames go up again with the overlap
        span = [(max(0, s - R), min(p.T, e + R)) for s, e in p.chunks]
        nxt = _prefetch(self.frames, span[0][0], span[0][1], self.up, vs.device)
        for c, (s, e) in enumerate(p.chunks):
            buf, ev = nxt
            if c + 1 < len(p.chunks):
                nxt = _prefetch(self.frames, span[c + 1][0], span[c + 1][1], self.up, vs.device)
            if ev is not None:
                self.compute.wait_event(ev)
            if R > 0:   # into a buffer of its own, which everything behind reads as the chunk's source
                lo = span[c][0]
                sharp = PF.deblur_frames(buf, self.dmaps[s:e], self.dgain[s:e], s - lo, e - lo, p.fmt.name, p.deblur_sensitivity)
                if p.on_host:
                    buf.record_stream(self.compute)
                buf = sharp
            fld = self.fields[s:e]
            if p.zmode is not None:
                fld = PF._field_zoom(fld, self.zcoef[s:e], (p.h, p.w), vs.align_corners, vs.interpolation, torch.empty_like(fld), self.zunc[s:e])
            self.finish(vs._warp(p.fmt, buf, fld), buf, s, e, self.compute)

    def measure(self):
        """metrics: every lane has joined the caller's stream, and every chunk's planes are behind an event it has waited for"""
        vs, p = self.vs, self.plan
        core = self.gray_all[p.halo_left:p.halo_left + p.T]
        vs.motion_in, vs.motion_inliers_in = global_motion(core)
        vs.motion_out, vs.motion_inliers_out = global_motion(self.planes_out)
        hom, bounds = (self.hom, self.bounds) if p.two_pass and p.lattice else (self.mhom, self.mbounds)
        vs._report = {"frames": p.T, "frame_hw": (p.h, p.w), "hom": hom, "bounds": bounds,
                      "cuts": [c - p.halo_left for c in self.cuts if 0 < c - p.halo_left < p.T]}
