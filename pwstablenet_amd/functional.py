"""Drop-in replacements for the torch functions the reference drivers call on the hot path
(reference main_new.py:106-118,195,197,706-716), backed by the HIP kernels through the C ABI.

Same names, argument meaning and defaults as ``torch.nn.functional``:
    grid_sample(input, grid, mode='bilinear', padding_mode='zeros', align_corners=None)
    affine_grid(theta, size, align_corners=None)
plus ``upsample_bilinear2d(x, size)`` (== ``torch.nn.UpsamplingBilinear2d(size=...)``) and the fused
``upsample_grid_sample(input, field)`` of the 720p path.  torch is used for device memory, streams and
autograd bookkeeping only.
"""
import torch

from . import hipabi as A


def _ac(align_corners):
    # torch >= 1.3 semantics, which is what the goldens were generated with: None -> False
    return 1 if align_corners else 0


class _GridSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, grid, align_corners):
        A.require_cuda(input, grid)
        if input.dim() != 4 or grid.dim() != 4 or grid.shape[-1] != 2 or grid.shape[0] != input.shape[0]:
            raise RuntimeError("grid_sample: expected input (N,C,H,W) and grid (N,Ho,Wo,2), got %s and %s"
                               % (tuple(input.shape), tuple(grid.shape)))
        input, grid = input.contiguous(), grid.contiguous()
        n, c, h, w = input.shape
        ho, wo = grid.shape[1], grid.shape[2]
        out = torch.empty((n, c, ho, wo), device=input.device, dtype=torch.float32)
        A.check(A.lib().pws_grid_sample_fwd(A.ptr(input), A.ptr(grid), A.ptr(out), n, c, h, w, ho, wo, align_corners,
                                            A.current_stream()), "pws_grid_sample_fwd")
        ctx.save_for_backward(input, grid)
        ctx.align_corners = align_corners
        return out

    @staticmethod
    def backward(ctx, gout):
        input, grid = ctx.saved_tensors
        gout = gout.contiguous()
        n, c, h, w = input.shape
        ho, wo = grid.shape[1], grid.shape[2]
        gi = torch.empty_like(input) if ctx.needs_input_grad[0] else None
        gg = torch.empty_like(grid) if ctx.needs_input_grad[1] else None
        A.check(A.lib().pws_grid_sample_bwd(A.ptr(gout), A.ptr(input), A.ptr(grid), A.ptr(gi), A.ptr(gg), n, c, h, w, ho,
                                            wo, ctx.align_corners, A.current_stream()), "pws_grid_sample_bwd")
        return gi, gg, None


def grid_sample(input, grid, mode="bilinear", padding_mode="zeros", align_corners=None):
    if mode != "bilinear" or padding_mode != "zeros":
        raise NotImplementedError("grid_sample: only mode='bilinear', padding_mode='zeros' (what the reference uses)")
    return _GridSample.apply(input, grid, _ac(align_corners))


class _AffineGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, n, h, w, align_corners):
        A.require_cuda(theta)
        theta = theta.contiguous().view(n, 6)
        grid = torch.empty((n, h, w, 2), device=theta.device, dtype=torch.float32)
        A.check(A.lib().pws_affine_grid(A.ptr(theta), A.ptr(grid), n, h, w, align_corners, A.current_stream()), "pws_affine_grid")
        ctx.dims = (n, h, w, align_corners)
        return grid

    @staticmethod
    def backward(ctx, ggrid):
        n, h, w, ac = ctx.dims
        ggrid = ggrid.contiguous()
        gtheta = torch.empty((n, 2, 3), device=ggrid.device, dtype=torch.float32)
        A.check(A.lib().pws_affine_grid_bwd(A.ptr(ggrid), A.ptr(gtheta), n, h, w, ac, A.current_stream()), "pws_affine_grid_bwd")
        return gtheta, None, None, None, None


def affine_grid(theta, size, align_corners=None):
    """F.affine_grid(theta (N,2,3), size (N,C,H,W)) -> (N,H,W,2) (reference lib/networks_cascading.py:164, main_new.py:195)."""
    A.require_cuda(theta)
    if len(size) != 4:
        raise NotImplementedError("affine_grid: 2-D grids only (size = (N, C, H, W))")
    n, h, w = int(size[0]), int(size[-2]), int(size[-1])
    if theta.numel() != n * 6:
        raise RuntimeError("affine_grid: expected theta of shape (%d, 2, 3), got %s" % (n, tuple(theta.shape)))
    return _AffineGrid.apply(theta, n, h, w, _ac(align_corners))


class _UpsampleBilinearAC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ho, wo):
        A.require_cuda(x)
        x = x.contiguous()
        n, c, h, w = x.shape
        out = torch.empty((n, c, ho, wo), device=x.device, dtype=torch.float32)
        A.check(A.lib().pws_upsample_bilinear_ac(A.ptr(x), A.ptr(out), n, c, h, w, ho, wo, A.current_stream()),
                "pws_upsample_bilinear_ac")
        ctx.dims = (n, c, h, w, ho, wo)
        return out

    @staticmethod
    def backward(ctx, gout):
        n, c, h, w, ho, wo = ctx.dims
        gout = gout.contiguous()
        gin = torch.empty((n, c, h, w), device=gout.device, dtype=torch.float32)
        A.check(A.lib().pws_upsample_bilinear_ac_bwd(A.ptr(gout), A.ptr(gin), n, c, h, w, ho, wo, A.current_stream()),
                "pws_upsample_bilinear_ac_bwd")
        return gin, None, None


def upsample_bilinear2d(x, size):
    """torch.nn.UpsamplingBilinear2d(size=size)(x): bilinear, align_corners=True (reference main_new.py:708)."""
    if x.dim() != 4:
        raise RuntimeError("upsample_bilinear2d: expected (N,C,H,W), got %s" % (tuple(x.shape),))
    if isinstance(size, int):
        size = (size, size)
    return _UpsampleBilinearAC.apply(x, int(size[0]), int(size[1]))


class UpsamplingBilinear2d(torch.nn.Module):
    def __init__(self, size=None, scale_factor=None):
        super().__init__()
        if size is None:
            raise NotImplementedError("UpsamplingBilinear2d: only size=(H, W) (what the reference uses)")
        self.size = size

    def forward(self, x):
        return upsample_bilinear2d(x, self.size)


INTERPOLATIONS = ("bilinear", "bicubic")


def _entry(mode, name):
    """The C entry point of a fused warp for ``mode``: the bilinear ``pws_upsample_grid_sample_<name>`` or its bicubic twin
    ``pws_upsample_grid_sample_bicubic_<name>`` (Keys cubic convolution, A = -0.75: torch's ``grid_sample(mode="bicubic")``; integer
    outputs are clamped to the format's range, then truncated).  Anything else is a ValueError, raised before the library is touched."""
    if mode not in INTERPOLATIONS:
        raise ValueError("mode must be one of %s, got %r" % (INTERPOLATIONS, mode))
    return "pws_upsample_grid_sample_" + ("bicubic_" if mode == "bicubic" else "") + name


def upsample_grid_sample(input, field, align_corners=None, mode="bilinear"):
    """grid_sample(input, UpsamplingBilinear2d(size=input.shape[-2:])(field)) without materialising the resized field.

    input: (N,C,H,W) frame; field: (N,h,w,2) warp field as returned by ``netG(x, False)``.  mode = "bicubic": the same warp with
    ``grid_sample(mode="bicubic")``'s 16 taps (forward only; W >= 4).
    """
    fn = _entry(mode, "fwd")
    A.require_cuda(input, field)
    input, field = input.contiguous(), field.contiguous()
    n, c, h, w = input.shape
    fh, fw = field.shape[1], field.shape[2]
    out = torch.empty_like(input)
    A.check(getattr(A.lib(), fn)(A.ptr(input), A.ptr(field), A.ptr(out), n, c, h, w, fh, fw, _ac(align_corners), A.current_stream()), fn)
    return out


def upsample_grid_sample_u8(frames_hwc, field, swap_rb=False, align_corners=None, out=None, mode="bilinear"):
    """The 720p step of the reference's ``process()`` on the frames as OpenCV delivers them (main_new.py:679-721):
    ``frames_hwc`` (N,H,W,3) uint8 -> [optional BGR<->RGB swap] -> float CHW -> grid_sample with the field resized to (H,W)
    (UpsamplingBilinear2d) -> ``astype(uint8)`` HWC, in one kernel and 6 bytes of frame traffic per pixel.  W % 4 == 0.
    mode = "bicubic": 16 taps per pixel (``grid_sample(mode="bicubic")``), the blend clamped to 0..255 before it is truncated."""
    fn = _entry(mode, "u8")
    A.require_cuda(field)
    A.require_cuda(frames_hwc, dtype=torch.uint8)
    if frames_hwc.dim() != 4 or frames_hwc.shape[3] != 3:
        raise ValueError("upsample_grid_sample_u8: frames must be uint8 (N,H,W,3), got %s %s" % (frames_hwc.dtype, tuple(frames_hwc.shape)))
    frames_hwc, field = frames_hwc.contiguous(), field.contiguous()
    n, h, w, _ = frames_hwc.shape
    if out is None:
        out = torch.empty_like(frames_hwc)
    A.check(getattr(A.lib(), fn)(A.ptr(frames_hwc), A.ptr(field), A.ptr(out), n, h, w, field.shape[1], field.shape[2],
                                 int(bool(swap_rb)), _ac(align_corners), A.current_stream()), fn)
    return out


PIXEL_FORMATS = ("bgr24", "nv12", "i420")
YUV420_LAYOUT = {"nv12": 0, "i420": 1}


def yuv420_layout(pixel_format):
    """0 (NV12) / 1 (I420) for an 8-bit 4:2:0 pixel format; ValueError for anything else (4:2:2, 4:4:4, full range and BT.709 are not
    supported; the 10-bit formats P010 / I010 have functions of their own: ``yuv420_16_layout``, ``yuv420_16_shape``,
    ``upsample_grid_sample_yuv420_16``)."""
    if pixel_format not in YUV420_LAYOUT:
        raise ValueError("pixel_format must be one of %s for 4:2:0 frames, got %r (8-bit BT.601 limited-range NV12 / I420 only)"
                         % (tuple(YUV420_LAYOUT), pixel_format))
    return YUV420_LAYOUT[pixel_format]


def yuv420_shape(frames, pixel_format, w_multiple=4):
    """(T, H, W) of packed 4:2:0 frames (T, H * 3 // 2, W) uint8; ValueError unless H and W are even and W a multiple of ``w_multiple``."""
    yuv420_layout(pixel_format)
    if frames.dim() != 3 or frames.dtype != torch.uint8:
        raise ValueError("%s frames must be uint8 (T, H * 3 // 2, W), got %s %s" % (pixel_format, frames.dtype, tuple(frames.shape)))
    t, ph, w = frames.shape
    if ph % 3 != 0 or ph == 0:
        raise ValueError("%s frames: packed height %d is not H * 3 // 2 of an even H" % (pixel_format, ph))
    h = ph // 3 * 2
    if w % 2 != 0 or w % w_multiple != 0:
        raise ValueError("%s frames: width %d must be even and a multiple of %d" % (pixel_format, w, w_multiple))
    return t, h, w


def upsample_grid_sample_yuv420(frames, field, pixel_format, align_corners=None, out=None, mode="bilinear"):
    """upsample_grid_sample_u8 for packed 4:2:0 frames, YUV in and YUV out: ``frames`` (N, H * 3 // 2, W) uint8 in ``pixel_format``
    "nv12" or "i420"; every plane is warped by ``field`` (N, fh, fw, 2) resized (align_corners=True) to the plane's own size, taps outside
    a plane read BT.601 black (16 in Y, 128 in U and V), the fp32 blend is truncated.  H even, W % 4 == 0.  One kernel launch.
    mode = "bicubic": 16 taps per sample, the blend clamped to 0..255 before it is truncated; W >= 8."""
    fn = _entry(mode, "yuv420_u8")
    A.require_cuda(field)
    A.require_cuda(frames, dtype=torch.uint8)
    layout = yuv420_layout(pixel_format)
    n, h, w = yuv420_shape(frames, pixel_format)
    if field.dim() != 4 or field.shape[0] != n or field.shape[3] != 2:
        raise ValueError("upsample_grid_sample_yuv420: field must be (%d, fh, fw, 2), got %s" % (n, tuple(field.shape)))
    frames, field = frames.contiguous(), field.contiguous()
    if out is None:
        out = torch.empty_like(frames)
    A.check(getattr(A.lib(), fn)(A.ptr(frames), A.ptr(field), A.ptr(out), n, h, w, field.shape[1], field.shape[2], layout,
                                 _ac(align_corners), A.current_stream()), fn)
    return out


PIXEL_FORMATS_16 = ("p010", "i010")
YUV420_16_LAYOUT = {"p010": 0, "i010": 1}


def yuv420_16_layout(pixel_format):
    """0 (P010: NV12's plane order, the 10-bit sample in the high bits of each 16-bit word) / 1 (I010, ffmpeg's yuv420p10le: I420's plane
    order, the sample in the low 10 bits) for a 10-bit 4:2:0 pixel format; ValueError for anything else."""
    if pixel_format not in YUV420_16_LAYOUT:
        raise ValueError("pixel_format must be one of %s for 10-bit 4:2:0 frames, got %r (BT.601 limited-range P010 / I010 only)"
                         % (tuple(YUV420_16_LAYOUT), pixel_format))
    return YUV420_16_LAYOUT[pixel_format]


def yuv420_16_shape(frames, pixel_format, w_multiple=4):
    """(T, H, W) of packed 10-bit 4:2:0 frames (T, H * 3 // 2, W) uint16; ValueError unless H and W are even and W a multiple of
    ``w_multiple``."""
    yuv420_16_layout(pixel_format)
    if frames.dim() != 3 or frames.dtype != torch.uint16:
        raise ValueError("%s frames must be uint16 (T, H * 3 // 2, W), got %s %s" % (pixel_format, frames.dtype, tuple(frames.shape)))
    t, ph, w = frames.shape
    if ph % 3 != 0 or ph == 0:
        raise ValueError("%s frames: packed height %d is not H * 3 // 2 of an even H" % (pixel_format, ph))
    h = ph // 3 * 2
    if w % 2 != 0 or w % w_multiple != 0:
        raise ValueError("%s frames: width %d must be even and a multiple of %d" % (pixel_format, w, w_multiple))
    return t, h, w


def upsample_grid_sample_yuv420_16(frames, field, pixel_format, align_corners=None, out=None, mode="bilinear"):
    """upsample_grid_sample_yuv420 for 10-bit frames, YUV in and YUV out: ``frames`` (N, H * 3 // 2, W) uint16 in ``pixel_format`` "p010"
    (sample = word >> 6; output words have zero low bits) or "i010" (sample = min(word, 1023)); every plane is warped by ``field``
    (N, fh, fw, 2) resized (align_corners=True) to the plane's own size, bilinear in fp32 on the 10-bit values, taps outside a plane read
    BT.601 black (64 in Y, 512 in U and V), the blend is truncated and clamped to 0..1023.  H even, W % 4 == 0.  One kernel launch.
    mode = "bicubic": 16 taps per sample on the 10-bit values, clamped to 0..1023, then truncated; W >= 8."""
    fn = _entry(mode, "yuv420_u16")
    layout = yuv420_16_layout(pixel_format)
    n, h, w = yuv420_16_shape(frames, pixel_format)   # (a tensor that is not uint16 is a ValueError, like a bad shape)
    A.require_cuda(field)
    A.require_cuda(frames, dtype=torch.uint16)
    if field.dim() != 4 or field.shape[0] != n or field.shape[3] != 2:
        raise ValueError("upsample_grid_sample_yuv420_16: field must be (%d, fh, fw, 2), got %s" % (n, tuple(field.shape)))
    frames, field = frames.contiguous(), field.contiguous()
    if out is None:
        out = torch.empty_like(frames)
    A.check(getattr(A.lib(), fn)(A.ptr(frames), A.ptr(field), A.ptr(out), n, h, w, field.shape[1], field.shape[2], layout,
                                 _ac(align_corners), A.current_stream()), fn)
    return out


BORDERS = ("black", "keep")


def keep_borders_(warped, field, initial, pixel_format="bgr24", initial_is_source=False, swap_rb=False, align_corners=None, mode="bilinear"):
    """vid.stab's ``crop=keep`` for the integer fused warps, IN PLACE on ``warped``: T consecutive warped frames of one scene ((T, H, W, 3)
    uint8 for "bgr24", packed (T, H * 3 // 2, W) uint8 for "nv12" / "i420", uint16 for "p010" / "i010"; contiguous) and the ``field``
    (T, fh, fw, 2) that warped them.  ``out[t] = covered ? warped[t] : out[t-1]`` per plane, where a pixel is covered iff its source position
    (the warp's own, bit for bit) satisfies ``m <= ix <= W-1-m`` and ``m <= iy <= H-1-m`` with m = 0 for mode "bilinear" (all 4 taps inside)
    and 1 for "bicubic" (all 16); NaN is not covered.  ``out[-1]`` is ``initial``, one frame of the frames' layout that does not overlap
    ``warped``: an earlier output frame, copied as it is, or -- ``initial_is_source`` -- a SOURCE frame read as the warp would write it
    (``swap_rb`` for BGR, P010 words masked to ``v10 << 6``, I010 words clamped to 1023).  Coverage is binary: every sample of the result is a
    copy of one of the two.  One launch (csrc/border_keep.hip).  Shape and alignment rules are the warps'.  Float frames are a ValueError.
    Returns ``warped``."""
    if mode not in INTERPOLATIONS:
        raise ValueError("mode must be one of %s, got %r" % (INTERPOLATIONS, mode))
    if not isinstance(warped, torch.Tensor) or warped.dtype not in (torch.uint8, torch.uint16):
        raise ValueError("keep_borders_: frames must be uint8 or uint16 (the integer pixel formats), got %s" % (getattr(warped, "dtype", type(warped)),))
    if pixel_format == "bgr24":
        if warped.dtype != torch.uint8 or warped.dim() != 4 or warped.shape[3] != 3:
            raise ValueError("keep_borders_: bgr24 frames must be uint8 (T,H,W,3), got %s %s" % (warped.dtype, tuple(warped.shape)))
        n, h, w = warped.shape[:3]
        fn, extra = "pws_border_keep_u8", int(bool(swap_rb))
    elif pixel_format in PIXEL_FORMATS_16:
        n, h, w = yuv420_16_shape(warped, pixel_format)
        fn, extra = "pws_border_keep_yuv420_u16", yuv420_16_layout(pixel_format)
    else:
        n, h, w = yuv420_shape(warped, pixel_format)   # (an unknown format, or a tensor that is not uint8, is a ValueError)
        fn, extra = "pws_border_keep_yuv420_u8", yuv420_layout(pixel_format)
    A.require_cuda(field)
    A.require_cuda(warped, initial, dtype=warped.dtype)
    if not warped.is_contiguous():
        raise ValueError("keep_borders_: frames are modified in place and must be contiguous")
    if tuple(initial.shape) != tuple(warped.shape[1:]):
        raise ValueError("keep_borders_: initial must be one frame %s, got %s" % (tuple(warped.shape[1:]), tuple(initial.shape)))
    if field.dim() != 4 or field.shape[0] != n or field.shape[3] != 2:
        raise ValueError("keep_borders_: field must be (%d, fh, fw, 2), got %s" % (n, tuple(field.shape)))
    field, initial = field.contiguous(), initial.contiguous()
    A.check(getattr(A.lib(), fn)(A.ptr(warped), A.ptr(field), A.ptr(initial), int(bool(initial_is_source)), n, h, w, field.shape[1],
                                 field.shape[2], extra, _ac(align_corners), int(mode == "bicubic"), A.current_stream()), fn)
    return warped


def adam_step_(p, g, m, v, lr, beta1, beta2, eps, step):
    """In-place fused Adam on flat fp32 CUDA buffers."""
    A.require_cuda(p, g, m, v)
    A.check(A.lib().pws_adam_step(A.ptr(p), A.ptr(g), A.ptr(m), A.ptr(v), p.numel(), lr, beta1, beta2, eps, step,
                                  A.current_stream()), "pws_adam_step")
