"""Frame I/O on the device: the window planes the generator reads, INTER_AREA resizes and crops of integer frames, every pixel format."""
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
