"""Drop-in replacements for the torch functions the reference drivers call on the hot path
(reference main_new.py:106-118,195,197,706-716), backed by the HIP kernels through the C ABI.

Same names, argument meaning and defaults as ``torch.nn.functional``:
    grid_sample(input, grid, mode='bilinear', padding_mode='zeros', align_corners=None)
    affine_grid(theta, size, align_corners=None)
plus ``upsample_bilinear2d(x, size)`` (== ``torch.nn.UpsamplingBilinear2d(size=...)``) and the fused
``upsample_grid_sample(input, field)`` of the 720p path.  torch is used for device memory, streams and
autograd bookkeeping only.
"""
import collections

import torch

from . import hipabi as A
from .scenes import _cut_list, _scenes


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


PIXEL_FORMATS = ("bgr24", "nv12", "i420")
YUV420_LAYOUT = {"nv12": 0, "i420": 1}
PIXEL_FORMATS_16 = ("p010", "i010")
YUV420_16_LAYOUT = {"p010": 0, "i010": 1}
BORDERS = ("black", "keep", "mosaic")   # which FRAMES may fill a wedge
EDGES = ("pad", "clamp", "mirror")       # how the SOURCE continues beyond its rim (the C entries' `edge`: the index)


CHROMA_SHIFTS = ((1, 1), (1, 0), (0, 0))   # (cx, cy) of chroma 0 (4:2:0), 1 (4:2:2), 2 (4:4:4): a chroma plane is (H >> cy) x (W >> cx)
_PACKED_ROWS = ("H * 3 // 2", "2 * H", "3 * H")


class FrameFormat(collections.namedtuple("FrameFormat", "name dtype packed layout suffix wrapper window_planes plane_resize chroma",
                                         defaults=(None,))):
    """What the warps, the keep pass and the stabiliser need to know about a pixel format, in one place: its ``name``, the frames' ``dtype``,
    whether they are ``packed`` YUV planes (T, packed rows, W) and then their plane ``layout`` (0: Y + interleaved UV, 1: Y + U + V; None for
    the unpacked formats) and ``chroma`` subsampling (0: 4:2:0, 1: 4:2:2, 2: 4:4:4; None for the unpacked formats), the ``suffix`` of the
    format's C entries (``pws_upsample_grid_sample_[bicubic_]<suffix>``, ``pws_border_keep_<suffix>``), the ``wrapper`` whose name its error
    messages carry, and the C entries that make its ``window_planes`` and resize its planes (``plane_resize``).  A new format is a row of
    FRAME_FORMATS -- the five formats of the 4:2:0 generation, whose names and order are pinned -- or of CHROMA_FORMATS (4:2:2 and 4:4:4),
    and its kernels; names are resolved through ``lookup_format``, which reads both tables."""
    __slots__ = ()

    @property
    def hwc(self):
        """(T, H, W, 3) frames ("bgr24"); the float frames are (T, C, H, W)."""
        return not self.packed and self.dtype == torch.uint8

    @property
    def shifts(self):
        """(cx, cy): a chroma plane of packed H x W frames is (H >> cy) x (W >> cx) samples; luma pixel (x, y) has chroma sample
        (x >> cx, y >> cy)."""
        return CHROMA_SHIFTS[self.chroma]

    @property
    def multiples(self):
        """(mx, my): what x and y edges of a window of packed frames must be multiples of, so that the window's chroma is whole samples."""
        cx, cy = self.shifts
        return 1 << cx, 1 << cy

    def packed_rows(self, h):
        """Rows of W samples that a packed frame of even height ``h`` takes: Y, then two chroma planes of (h >> cy) x (W >> cx)."""
        cx, cy = self.shifts
        return h + ((2 * (h >> cy)) >> cx)

    def frame_shape(self, frames, w_multiple=4):
        """(T, H, W) of ``frames``.  Packed frames: (T, packed_rows(H), W) of the format's dtype -- H * 3 // 2 rows for 4:2:0, 2 * H for 4:2:2,
        3 * H for 4:4:4 -- ValueError unless H and W are even and W a multiple of ``w_multiple``.  Unpacked frames are read by position,
        (T, H, W, 3) or float (T, C, H, W): only another rank is a ValueError here (dtype, channel count and width are checked where the
        frames are used, behind the check for host tensors)."""
        if not self.packed:
            if frames.dim() != 4:
                raise ValueError("%s: frames must be %s, got %s %s" % (self.wrapper, "uint8 (N,H,W,3)" if self.hwc else "float32 (N,C,H,W)",
                                                                     frames.dtype, tuple(frames.shape)))
            return (frames.shape[0],) + tuple(frames.shape[1:3] if self.hwc else frames.shape[2:4])
        rows = _PACKED_ROWS[self.chroma]
        if frames.dim() != 3 or frames.dtype != self.dtype:
            raise ValueError("%s frames must be %s (T, %s, W), got %s %s" % (self.name, str(self.dtype)[6:], rows, frames.dtype, tuple(frames.shape)))
        t, ph, w = frames.shape
        unit = self.packed_rows(2)   # (the packed rows of two picture rows: 3, 4, 6)
        if ph % unit != 0 or ph == 0:
            raise ValueError("%s frames: packed height %d is not %s of an even H" % (self.name, ph, rows))
        h = ph // unit * 2
        if w % 2 != 0 or w % w_multiple != 0:
            raise ValueError("%s frames: width %d must be even and a multiple of %d" % (self.name, w, w_multiple))
        return t, h, w

    def planes(self, x, h, w):
        """Views of the planes of packed frames x (T, packed_rows(h), w): [Y (T, h, w), UV (T, h >> cy, 2 * (w >> cx))] for layout 0 (U V
        interleaved), [Y, U, V] with U and V (T, h >> cy, w >> cx) for layout 1."""
        cx, cy = self.shifts
        t = x.shape[0]
        y = x[:, :h]
        if self.layout == 0:
            return [y, x[:, h:]]   # (4:2:0 and 4:2:2: a row of w >> 1 pairs is w samples)
        c = x.reshape(t, -1)[:, h * w:].reshape(t, 2, h >> cy, w >> cx)
        return [y, c[:, 0], c[:, 1]]

    def extra(self, flag=False):
        """The first format argument of the C entries: the plane layout of packed frames; for BGR the caller's ``flag`` (swap_rb, frames_are_rgb)."""
        return self.layout if self.packed else int(bool(flag))

    def args(self, flag=False):
        """The format arguments of the C entries, in their order: ``extra(flag)``, and for the entries that take it (the 4:2:2 / 4:4:4
        formats' ``*_yuv_*``) the chroma subsampling behind it.  The ``*_yuv420_*`` entries take the layout alone."""
        return (self.extra(flag),) + ((self.chroma,) if self.chroma else ())

    def warp_entry(self, mode):
        return _entry(mode, self.suffix)

    @property
    def keep_entry(self):
        return "pws_border_keep_" + self.suffix

    @property
    def mosaic_entry(self):
        """The format's mosaic pass: one entry per sample size for every packed YUV format (``chroma`` is always passed), one for BGR."""
        return "pws_border_mosaic_" + ("u8" if not self.packed else "yuv_u16" if self.dtype == torch.uint16 else "yuv_u8")

    @property
    def edge_entry(self):
        """The format's edge pass: as ``mosaic_entry``, one entry per sample size for every packed YUV format, one for BGR."""
        return "pws_border_edge_" + ("u8" if not self.packed else "yuv_u16" if self.dtype == torch.uint16 else "yuv_u8")


FRAME_FORMATS = {f.name: f for f in (
    FrameFormat("bgr24", torch.uint8, False, None, "u8", "upsample_grid_sample_u8", "pws_gray_area_u8", "pws_area_resize_u8"),
    FrameFormat("nv12", torch.uint8, True, 0, "yuv420_u8", "upsample_grid_sample_yuv420", "pws_gray_area_yuv420_u8", "pws_area_resize_plane_u8", 0),
    FrameFormat("i420", torch.uint8, True, 1, "yuv420_u8", "upsample_grid_sample_yuv420", "pws_gray_area_yuv420_u8", "pws_area_resize_plane_u8", 0),
    FrameFormat("p010", torch.uint16, True, 0, "yuv420_u16", "upsample_grid_sample_yuv420_16", "pws_gray_area_yuv420_u16", "pws_area_resize_plane_u16", 0),
    FrameFormat("i010", torch.uint16, True, 1, "yuv420_u16", "upsample_grid_sample_yuv420_16", "pws_gray_area_yuv420_u16", "pws_area_resize_plane_u16", 0),
)}
# 4:2:2 and 4:4:4, named the libyuv way (ffmpeg: nv16, yuv422p, p210le, yuv422p10le, yuv444p, yuv444p10le): a table of their own, FRAME_FORMATS
# being pinned to the five above.  Interleaved 4:4:4 (NV24 / P410) is not offered.
CHROMA_FORMATS = {f.name: f for f in (
    FrameFormat("nv16", torch.uint8, True, 0, "yuv_u8", "upsample_grid_sample_yuv", "pws_gray_area_yuv_u8", "pws_area_resize_plane_u8", 1),
    FrameFormat("i422", torch.uint8, True, 1, "yuv_u8", "upsample_grid_sample_yuv", "pws_gray_area_yuv_u8", "pws_area_resize_plane_u8", 1),
    FrameFormat("p210", torch.uint16, True, 0, "yuv_u16", "upsample_grid_sample_yuv", "pws_gray_area_yuv_u16", "pws_area_resize_plane_u16", 1),
    FrameFormat("i210", torch.uint16, True, 1, "yuv_u16", "upsample_grid_sample_yuv", "pws_gray_area_yuv_u16", "pws_area_resize_plane_u16", 1),
    FrameFormat("i444", torch.uint8, True, 1, "yuv_u8", "upsample_grid_sample_yuv", "pws_gray_area_yuv_u8", "pws_area_resize_plane_u8", 2),
    FrameFormat("i410", torch.uint16, True, 1, "yuv_u16", "upsample_grid_sample_yuv", "pws_gray_area_yuv_u16", "pws_area_resize_plane_u16", 2),
)}
PACKED_FORMATS = tuple(n for n in FRAME_FORMATS if FRAME_FORMATS[n].packed) + tuple(CHROMA_FORMATS)   # every packed YUV format, both depths
# the float (T, C, H, W) frames that run() accepts under "bgr24": no keep pass, no window planes, no resize
_FLOAT_FRAMES = FrameFormat("bgr24", torch.float32, False, None, "fwd", "upsample_grid_sample", None, None)


def lookup_format(pixel_format):
    """The record that ``pixel_format`` names in FRAME_FORMATS or CHROMA_FORMATS, or None: the one place where a name becomes a record."""
    try:
        return FRAME_FORMATS.get(pixel_format) or CHROMA_FORMATS.get(pixel_format)
    except TypeError:   # (an unhashable "name")
        return None


def _packed_format(pixel_format, dtype):
    """The record of a packed 4:2:0 format of that sample dtype; ValueError for any other name."""
    fmt = FRAME_FORMATS.get(pixel_format)
    if fmt is None or not fmt.packed or fmt.dtype != dtype:
        if dtype == torch.uint8:
            raise ValueError("pixel_format must be one of %s for 4:2:0 frames, got %r (8-bit BT.601 limited-range NV12 / I420 only)"
                             % (tuple(YUV420_LAYOUT), pixel_format))
        raise ValueError("pixel_format must be one of %s for 10-bit 4:2:0 frames, got %r (BT.601 limited-range P010 / I010 only)"
                         % (tuple(YUV420_16_LAYOUT), pixel_format))
    return fmt


def _yuv_format(pixel_format, dtype=None):
    """The record of any packed YUV format (of that sample dtype, if one is given); ValueError for any other name."""
    fmt = lookup_format(pixel_format)
    if fmt is None or not fmt.packed or (dtype is not None and fmt.dtype != dtype):
        names = tuple(n for n in PACKED_FORMATS if dtype is None or lookup_format(n).dtype == dtype)
        raise ValueError("pixel_format must be one of %s for packed %sYUV frames, got %r (BT.601 limited range)"
                         % (names, {None: "", torch.uint8: "8-bit ", torch.uint16: "10-bit "}[dtype], pixel_format))
    return fmt


def frame_format(pixel_format, frames, what, float_frames=False):
    """The record that ``pixel_format`` names, for ``frames``; packed frames are checked against it (``FrameFormat.frame_shape``).  A name that
    is in neither table (``lookup_format``) is ``yuv420_layout``'s ValueError; uint16 frames under "bgr24" are a ValueError naming ``what``; float_frames:
    "bgr24" frames that are not uint8 are float (T, C, H, W) frames."""
    fmt = lookup_format(pixel_format) or _packed_format(pixel_format, torch.uint8)
    if fmt.packed:
        fmt.frame_shape(frames)
    elif frames.dtype == torch.uint16:
        raise ValueError("%s: uint16 frames need pixel_format \"p010\" or \"i010\", got %r" % (what, pixel_format))
    elif float_frames and frames.dtype != torch.uint8:
        fmt = _FLOAT_FRAMES
    return fmt


def warp(frames, field, fmt, swap_rb=False, align_corners=None, out=None, mode="bilinear"):
    """The fused resize + warp of ``frames`` in the format ``fmt`` (a FrameFormat) by ``field`` (N, fh, fw, 2): the one implementation behind
    ``upsample_grid_sample``, ``upsample_grid_sample_u8``, ``upsample_grid_sample_yuv420``, ``upsample_grid_sample_yuv420_16`` and
    ``upsample_grid_sample_yuv``, which
    document what each format computes.  An invalid ``mode`` is raised before anything else, then the format's shape rules (ValueError),
    then host tensors or a wrong dtype (RuntimeError).  ``swap_rb`` applies to "bgr24" alone."""
    fn = fmt.warp_entry(mode)
    n, h, w = fmt.frame_shape(frames)
    A.require_cuda(field)
    A.require_cuda(frames, dtype=fmt.dtype)
    if fmt.hwc and frames.shape[3] != 3:
        raise ValueError("%s: frames must be uint8 (N,H,W,3), got %s %s" % (fmt.wrapper, frames.dtype, tuple(frames.shape)))
    if fmt.packed and (field.dim() != 4 or field.shape[0] != n or field.shape[3] != 2):
        raise ValueError("%s: field must be (%d, fh, fw, 2), got %s" % (fmt.wrapper, n, tuple(field.shape)))
    frames, field = frames.contiguous(), field.contiguous()
    if out is None:
        out = torch.empty_like(frames)
    integer = fmt.packed or fmt.hwc   # (the float entry takes the channel count and no format argument)
    shape = (n, h, w) if integer else (n, frames.shape[1], h, w)
    extra = fmt.args(swap_rb) if integer else ()
    A.check(getattr(A.lib(), fn)(A.ptr(frames), A.ptr(field), A.ptr(out), *shape, field.shape[1], field.shape[2], *extra, _ac(align_corners),
                                 A.current_stream()), fn)
    return out


def upsample_grid_sample(input, field, align_corners=None, mode="bilinear"):
    """grid_sample(input, UpsamplingBilinear2d(size=input.shape[-2:])(field)) without materialising the resized field.

    input: (N,C,H,W) frame; field: (N,h,w,2) warp field as returned by ``netG(x, False)``.  mode = "bicubic": the same warp with
    ``grid_sample(mode="bicubic")``'s 16 taps (forward only; W >= 4).
    """
    _entry(mode, "fwd")
    A.require_cuda(input, field)
    return warp(input, field, _FLOAT_FRAMES, align_corners=align_corners, mode=mode)


def upsample_grid_sample_u8(frames_hwc, field, swap_rb=False, align_corners=None, out=None, mode="bilinear"):
    """The 720p step of the reference's ``process()`` on the frames as OpenCV delivers them (main_new.py:679-721):
    ``frames_hwc`` (N,H,W,3) uint8 -> [optional BGR<->RGB swap] -> float CHW -> grid_sample with the field resized to (H,W)
    (UpsamplingBilinear2d) -> ``astype(uint8)`` HWC, in one kernel and 6 bytes of frame traffic per pixel.  W % 4 == 0.
    mode = "bicubic": 16 taps per pixel (``grid_sample(mode="bicubic")``), the blend clamped to 0..255 before it is truncated."""
    _entry(mode, "u8")
    A.require_cuda(field)
    A.require_cuda(frames_hwc, dtype=torch.uint8)   # (a host tensor or another dtype wins over a bad shape here, as it always has)
    return warp(frames_hwc, field, FRAME_FORMATS["bgr24"], swap_rb, align_corners, out, mode)


def yuv420_layout(pixel_format):
    """0 (NV12) / 1 (I420) for an 8-bit 4:2:0 pixel format; ValueError for anything else (4:2:2 and 4:4:4 have formats of their own,
    CHROMA_FORMATS, behind ``upsample_grid_sample_yuv`` and ``yuv_shape``; full range and BT.709 are not supported; the 10-bit formats P010 / I010 have functions of their own: ``yuv420_16_layout``, ``yuv420_16_shape``,
    ``upsample_grid_sample_yuv420_16``)."""
    return _packed_format(pixel_format, torch.uint8).layout


def yuv420_shape(frames, pixel_format, w_multiple=4):
    """(T, H, W) of packed 4:2:0 frames (T, H * 3 // 2, W) uint8; ValueError unless H and W are even and W a multiple of ``w_multiple``."""
    return _packed_format(pixel_format, torch.uint8).frame_shape(frames, w_multiple)


def upsample_grid_sample_yuv420(frames, field, pixel_format, align_corners=None, out=None, mode="bilinear"):
    """upsample_grid_sample_u8 for packed 4:2:0 frames, YUV in and YUV out: ``frames`` (N, H * 3 // 2, W) uint8 in ``pixel_format``
    "nv12" or "i420"; every plane is warped by ``field`` (N, fh, fw, 2) resized (align_corners=True) to the plane's own size, taps outside
    a plane read BT.601 black (16 in Y, 128 in U and V), the fp32 blend is truncated.  H even, W % 4 == 0.  One kernel launch.
    mode = "bicubic": 16 taps per sample, the blend clamped to 0..255 before it is truncated; W >= 8."""
    _entry(mode, "yuv420_u8")
    A.require_cuda(field)
    A.require_cuda(frames, dtype=torch.uint8)   # (wins over the format's name and shape rules here, as it always has)
    return warp(frames, field, _packed_format(pixel_format, torch.uint8), False, align_corners, out, mode)


def yuv420_16_layout(pixel_format):
    """0 (P010: NV12's plane order, the 10-bit sample in the high bits of each 16-bit word) / 1 (I010, ffmpeg's yuv420p10le: I420's plane
    order, the sample in the low 10 bits) for a 10-bit 4:2:0 pixel format; ValueError for anything else."""
    return _packed_format(pixel_format, torch.uint16).layout


def yuv420_16_shape(frames, pixel_format, w_multiple=4):
    """(T, H, W) of packed 10-bit 4:2:0 frames (T, H * 3 // 2, W) uint16; ValueError unless H and W are even and W a multiple of
    ``w_multiple``."""
    return _packed_format(pixel_format, torch.uint16).frame_shape(frames, w_multiple)


def upsample_grid_sample_yuv420_16(frames, field, pixel_format, align_corners=None, out=None, mode="bilinear"):
    """upsample_grid_sample_yuv420 for 10-bit frames, YUV in and YUV out: ``frames`` (N, H * 3 // 2, W) uint16 in ``pixel_format`` "p010"
    (sample = word >> 6; output words have zero low bits) or "i010" (sample = min(word, 1023)); every plane is warped by ``field``
    (N, fh, fw, 2) resized (align_corners=True) to the plane's own size, bilinear in fp32 on the 10-bit values, taps outside a plane read
    BT.601 black (64 in Y, 512 in U and V), the blend is truncated and clamped to 0..1023.  H even, W % 4 == 0.  One kernel launch.
    mode = "bicubic": 16 taps per sample on the 10-bit values, clamped to 0..1023, then truncated; W >= 8."""
    _entry(mode, "yuv420_u16")   # (then the format's name, then shape and dtype -- a tensor that is not uint16 is a ValueError -- then require_cuda)
    return warp(frames, field, _packed_format(pixel_format, torch.uint16), False, align_corners, out, mode)


def yuv_shape(frames, pixel_format, w_multiple=4):
    """(T, H, W) of packed YUV frames in any packed ``pixel_format`` (PACKED_FORMATS), of its dtype: (T, H * 3 // 2, W) for the 4:2:0 formats,
    (T, 2 * H, W) for "nv16" / "i422" / "p210" / "i210", (T, 3 * H, W) for "i444" / "i410"; ValueError unless H and W are even and W a
    multiple of ``w_multiple``."""
    return _yuv_format(pixel_format).frame_shape(frames, w_multiple)


def upsample_grid_sample_yuv(frames, field, pixel_format, align_corners=None, out=None, mode="bilinear"):
    """The fused warp for packed YUV frames of ANY packed format, YUV in and YUV out.  The 4:2:0 names give the bits of
    ``upsample_grid_sample_yuv420`` / ``upsample_grid_sample_yuv420_16``.  4:2:2 -- "nv16" (Y, then H rows of W/2 interleaved U V pairs) and
    "i422" (Y, U, V with H x W/2 chroma planes), uint8 (N, 2 * H, W); "p210" / "i210", the same in uint16 words placed as P010's / I010's -- and
    4:4:4 -- "i444" uint8, "i410" uint16 (low 10 bits), (N, 3 * H, W): Y, U, V planes of H x W.  Every plane is warped by ``field``
    (N, fh, fw, 2) resized (align_corners=True) to the plane's OWN size (chroma is taken as centred on its own grid), taps outside a plane read
    BT.601 limited-range black (16 / 128; 64 / 512 at 10 bits), the fp32 blend is truncated (10 bits: and clamped to 0..1023).  A plane comes
    out bit for bit as the same-sized plane of a 4:2:0 frame does.  H even, W % 4 == 0 for every format.  One kernel launch.
    mode = "bicubic": 16 taps per sample, clamped to the sample range, then truncated; the chroma planes hold the 4-tap window: W >= 8, any W
    for 4:4:4."""
    if mode not in INTERPOLATIONS:
        raise ValueError("mode must be one of %s, got %r" % (INTERPOLATIONS, mode))
    return warp(frames, field, _yuv_format(pixel_format), False, align_corners, out, mode)   # (name, then shape and dtype, then require_cuda)


def keep_borders_(warped, field, initial, pixel_format="bgr24", initial_is_source=False, swap_rb=False, align_corners=None, mode="bilinear"):
    """vid.stab's ``crop=keep`` for the integer fused warps, IN PLACE on ``warped``: T consecutive warped frames of one scene ((T, H, W, 3)
    uint8 for "bgr24", packed (T, H * 3 // 2, W) uint8 for "nv12" / "i420", uint16 for "p010" / "i010", the 4:2:2 and 4:4:4 formats of
    CHROMA_FORMATS in their packed shapes; contiguous) and the ``field``
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
    fmt = lookup_format(pixel_format) or _packed_format(pixel_format, torch.uint8)   # (an unknown format is a ValueError)
    if fmt.hwc and (warped.dtype != torch.uint8 or warped.dim() != 4 or warped.shape[3] != 3):
        raise ValueError("keep_borders_: bgr24 frames must be uint8 (T,H,W,3), got %s %s" % (warped.dtype, tuple(warped.shape)))
    n, h, w = fmt.frame_shape(warped)   # (packed frames: a tensor of the other depth's dtype is a ValueError)
    fn = fmt.keep_entry
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
                                 field.shape[2], *fmt.args(swap_rb), _ac(align_corners), int(mode == "bicubic"), A.current_stream()), fn)
    return warped


MOSAIC_MAX_RADIUS = 15   # (one window bit per frame, 2 radius + 1 of them in a 32-bit register)


def mosaic_borders_(warped, field, radius, start=0, stop=None, pixel_format="bgr24", align_corners=None, mode="bilinear", return_unfilled=False,
                    _unfilled=None):
    """Mosaic borders for the integer fused warps, IN PLACE on ``warped``: n consecutive frames of one scene as the black-border warp wrote
    them (``keep_borders_``' shapes and formats; contiguous) and the ``field`` (n, fh, fw, 2) that warped them.  Planes, source positions and
    coverage are ``keep_borders_``': a position is covered iff ``m <= ix <= W-1-m`` and ``m <= iy <= H-1-m``, m = 0 for mode "bilinear", 1 for
    "bicubic"; NaN is not covered.  Frames ``[start, stop)`` (``stop=None``: n) are filled, all n frames are donors: an uncovered position p of
    frame t takes the sample of the temporally nearest frame that covers p -- k = 1 .. ``radius``, frame t-k first (the past wins a tie), then
    frame t+k, inside [0, n).  Without a donor within ``radius`` (1 .. 15) the warp's blend with the pad colour stays, and the position counts
    as unfilled.  Covered samples are never modified and donors are read only where they are covered, so the result for [start, stop)
    depends on frames [start-radius, stop+radius) alone and chunked calls give the bytes of one call.  One launch (csrc/border_mosaic.hip).
    Float frames are a ValueError.  Returns ``warped``, or with ``return_unfilled`` ``(warped, unfilled)``: (stop - start,) int32 on the
    device, per frame the Y-plane (BGR: pixel) positions without a donor."""
    if mode not in INTERPOLATIONS:
        raise ValueError("mode must be one of %s, got %r" % (INTERPOLATIONS, mode))
    if not isinstance(warped, torch.Tensor) or warped.dtype not in (torch.uint8, torch.uint16):
        raise ValueError("mosaic_borders_: frames must be uint8 or uint16 (the integer pixel formats), got %s" % (getattr(warped, "dtype", type(warped)),))
    fmt = lookup_format(pixel_format) or _packed_format(pixel_format, torch.uint8)   # (an unknown format is a ValueError)
    if fmt.hwc and (warped.dtype != torch.uint8 or warped.dim() != 4 or warped.shape[3] != 3):
        raise ValueError("mosaic_borders_: bgr24 frames must be uint8 (T,H,W,3), got %s %s" % (warped.dtype, tuple(warped.shape)))
    n, h, w = fmt.frame_shape(warped)   # (packed frames: a tensor of the other depth's dtype is a ValueError)
    radius, start, stop = int(radius), int(start), n if stop is None else int(stop)
    if not 1 <= radius <= MOSAIC_MAX_RADIUS:
        raise ValueError("mosaic_borders_: radius must be 1 .. %d (one window bit per frame), got %d" % (MOSAIC_MAX_RADIUS, radius))
    if not 0 <= start <= stop <= n:
        raise ValueError("mosaic_borders_: the range must satisfy 0 <= start <= stop <= %d, got [%d, %d)" % (n, start, stop))
    fn = fmt.mosaic_entry
    A.require_cuda(field)
    A.require_cuda(warped, dtype=warped.dtype)
    if not warped.is_contiguous():
        raise ValueError("mosaic_borders_: frames are modified in place and must be contiguous")
    if field.dim() != 4 or field.shape[0] != n or field.shape[3] != 2:
        raise ValueError("mosaic_borders_: field must be (%d, fh, fw, 2), got %s" % (n, tuple(field.shape)))
    field = field.contiguous()
    # (_unfilled, the stabiliser's: the contiguous (stop - start,) int32 slice of its per-clip counts to write into)
    unfilled = _unfilled if _unfilled is not None else torch.empty(stop - start, dtype=torch.int32, device=warped.device)
    fargs = (fmt.layout, fmt.chroma) if fmt.packed else ()
    A.check(getattr(A.lib(), fn)(A.ptr(warped), A.ptr(field), A.ptr(unfilled), n, start, stop, radius, h, w, field.shape[1], field.shape[2], *fargs,
                                 _ac(align_corners), int(mode == "bicubic"), A.current_stream()), fn)
    return (warped, unfilled) if return_unfilled else warped


def edge_borders_(warped, source, field, edge, pixel_format="bgr24", swap_rb=False, align_corners=None, mode="bilinear"):
    """Edge modes for the integer fused warps, IN PLACE on ``warped``: n frames as the black-border warp wrote them (``keep_borders_``' shapes
    and formats; contiguous), the n ``source`` frames they were warped from (same shape and dtype, not overlapping ``warped``) and the
    ``field`` (n, fh, fw, 2) that warped them.  Planes, source positions and coverage are ``keep_borders_``': a position is covered iff
    ``m <= ix <= W-1-m`` and ``m <= iy <= H-1-m``, m = 0 for mode "bilinear", 1 for "bicubic"; NaN is not covered.  A covered sample keeps the
    warp's bytes, and so does one with a non-finite coordinate.  Every other sample is replaced whole by the source plane sampled at
    (ix, iy) with ``mode``'s taps (2 x 2, or 4 x 4 with the Keys weights, A = -0.75) and the plane continued beyond its rim: ``edge`` "clamp"
    repeats the edge sample (tap index ``min(max(i, 0), n-1)``: torch's ``padding_mode="border"``, OpenCV's BORDER_REPLICATE), "mirror"
    reflects about it without repeating it (``k = i mod 2(n-1)``, ``k < n ? k : 2(n-1) - k``: "reflection" with align_corners=True,
    BORDER_REFLECT_101).  Source samples are read as the warp reads them (``swap_rb``; P010 ``word >> 6``; I010 ``min(word, 1023)``), the
    fp32 blend is clamped to the sample range, truncated and written as the warp writes it.  Taps that all hold one value give that value
    exactly, and every finite coordinate is defined.  "pad" returns ``warped`` as it is, without a launch.  No other frame is read.  One
    launch (csrc/border_edge.hip).  Float frames, a non-contiguous ``warped``, a ``source`` of another shape or dtype and an unknown ``edge``
    or ``mode`` are ValueErrors.  Returns ``warped``."""
    if mode not in INTERPOLATIONS:
        raise ValueError("mode must be one of %s, got %r" % (INTERPOLATIONS, mode))
    if not isinstance(edge, str) or edge not in EDGES:
        raise ValueError("edge must be one of %s, got %r" % (EDGES, edge))
    if not isinstance(warped, torch.Tensor) or warped.dtype not in (torch.uint8, torch.uint16):
        raise ValueError("edge_borders_: frames must be uint8 or uint16 (the integer pixel formats), got %s" % (getattr(warped, "dtype", type(warped)),))
    fmt = lookup_format(pixel_format) or _packed_format(pixel_format, torch.uint8)   # (an unknown format is a ValueError)
    if fmt.hwc and (warped.dtype != torch.uint8 or warped.dim() != 4 or warped.shape[3] != 3):
        raise ValueError("edge_borders_: bgr24 frames must be uint8 (T,H,W,3), got %s %s" % (warped.dtype, tuple(warped.shape)))
    n, h, w = fmt.frame_shape(warped)   # (packed frames: a tensor of the other depth's dtype is a ValueError)
    if not isinstance(source, torch.Tensor) or source.dtype != warped.dtype or tuple(source.shape) != tuple(warped.shape):
        raise ValueError("edge_borders_: source must be the warped frames' sources, %s %s, got %s %s"
                         % (warped.dtype, tuple(warped.shape), getattr(source, "dtype", type(source)), tuple(getattr(source, "shape", ()))))
    if not warped.is_contiguous():
        raise ValueError("edge_borders_: frames are modified in place and must be contiguous")
    if edge == "pad":
        return warped
    fn = fmt.edge_entry
    A.require_cuda(field)
    A.require_cuda(warped, source, dtype=warped.dtype)
    if field.dim() != 4 or field.shape[0] != n or field.shape[3] != 2:
        raise ValueError("edge_borders_: field must be (%d, fh, fw, 2), got %s" % (n, tuple(field.shape)))
    field, source = field.contiguous(), source.contiguous()
    fargs = (fmt.layout, fmt.chroma) if fmt.packed else (int(bool(swap_rb)),)
    A.check(getattr(A.lib(), fn)(A.ptr(warped), A.ptr(source), A.ptr(field), n, h, w, field.shape[1], field.shape[2], *fargs, _ac(align_corners),
                                 int(mode == "bicubic"), EDGES.index(edge), A.current_stream()), fn)
    return warped


DEBLUR_MAX_RADIUS = 15   # frames: the generator's own window of +-15 frames at period 30, and mosaic_borders_' reach


def _check_deblur(radius, sensitivity, what, zero_ok=False):
    """(R, s): ``radius`` as an int in 1 .. 15 (or 0 .. 15) and ``sensitivity`` as a finite positive float; ValueError otherwise (NaN included)."""
    try:
        r = int(radius)
        whole = not isinstance(radius, bool) and r == radius
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or not (0 if zero_ok else 1) <= r <= DEBLUR_MAX_RADIUS:
        raise ValueError("%s: the deblur radius must be a whole number of frames in %d .. %d, got %r" % (what, 0 if zero_ok else 1, DEBLUR_MAX_RADIUS, radius))
    try:
        s = float(sensitivity)
    except (TypeError, ValueError):
        raise ValueError("%s: the deblur sensitivity must be a number of gray levels, got %r" % (what, sensitivity)) from None
    if not (0.0 < s < float("inf")) or s > 3.0e38:
        raise ValueError("%s: the deblur sensitivity must be finite and positive, got %r" % (what, sensitivity))
    return r, s


def deblur_frames(frames, maps, gain, start=0, stop=None, pixel_format="bgr24", sensitivity=4.0, out=None):
    """Deblurring for the integer pixel formats (OpenCV videostab's ``WeightingDeblurer`` with bilinear donors; csrc/deblur.hip;
    include/pwstable.h pws_deblur_u8 has the definition in full): ``frames``, n consecutive SOURCE frames of one clip (``keep_borders_``'
    shapes and formats), and the plan's rows for frames ``[start, stop)`` (``stop=None``: n) -- ``maps`` (stop - start, 2R+1, 6) float64 and
    ``gain`` (stop - start, 2R+1) float32 as ``stream.deblur_plan`` returns them, on the device.  Returns the stop - start deblurred frames, in
    a fresh tensor or in ``out`` (same layout, not overlapping ``frames``).  Per sample position p of frame t: the frame's own sample with
    weight 1, and for k = -R .. -1, 1 .. R with ``gain[t, k] > 0`` and frame t+k inside [0, n), the donor frame sampled bilinearly (fp32) at
    ``q = maps[t, k] (p - centre) + centre`` -- fp64, rounded once to fp32, used only where 0 <= qx <= W-1 and 0 <= qy <= H-1 -- with weight
    ``gain * s / (s + |I_q - I_0|)``: s = ``sensitivity`` in 8-bit gray levels (times 4 for the 10-bit formats), I the sample for YUV and
    (29 B + 150 G + 77 R) / 256 for BGR, whose three channels share the weight.  The weighted mean is rounded to the nearest integer and
    clamped to the sample range (P010 / P210 words are written back ``<< 6``).  Packed YUV frames have their LUMA blended and their chroma
    planes copied: blur detail lives in luma.  A frame without donors is a copy.  Every read is of ``frames``, so chunked calls over a clip
    padded by R frames give the bytes of one call (``mosaic_borders_``' property).
    The sensitivity guards against donors that do not show the same thing -- parallax, moving objects, a motion fit that is off: a donor
    s gray levels away gets half its gain.  The default 4.0 is a judgement that no footage here can fit, like ``zoom_speed``: OpenCV's 0.1
    lends almost nothing on the synthetic clip of tests/test_deblur_ref_cpu.py.  One launch.
    ValueError: float frames, host tensors, shapes or dtypes that do not fit, a range outside 0 <= start <= stop <= n, R outside 1 .. 15, a
    sensitivity that is not finite and positive."""
    if not isinstance(frames, torch.Tensor) or frames.dtype not in (torch.uint8, torch.uint16):
        raise ValueError("deblur_frames: frames must be uint8 or uint16 (the integer pixel formats), got %s" % (getattr(frames, "dtype", type(frames)),))
    fmt = lookup_format(pixel_format) or _packed_format(pixel_format, torch.uint8)   # (an unknown format is a ValueError)
    if fmt.hwc and (frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3):
        raise ValueError("deblur_frames: bgr24 frames must be uint8 (T,H,W,3), got %s %s" % (frames.dtype, tuple(frames.shape)))
    n, h, w = fmt.frame_shape(frames)   # (packed frames: a tensor of the other depth's dtype is a ValueError)
    start, stop = int(start), n if stop is None else int(stop)
    if not 0 <= start <= stop <= n:
        raise ValueError("deblur_frames: the range must satisfy 0 <= start <= stop <= %d, got [%d, %d)" % (n, start, stop))
    m = stop - start
    if (not isinstance(maps, torch.Tensor) or maps.dtype != torch.float64 or maps.dim() != 3 or maps.shape[0] != m or maps.shape[2] != 6
            or maps.shape[1] % 2 != 1):
        raise ValueError("deblur_frames: maps must be (%d, 2R+1, 6) float64, got %s %s" % (m, getattr(maps, "dtype", type(maps)), tuple(getattr(maps, "shape", ()))))
    k = maps.shape[1]
    if not isinstance(gain, torch.Tensor) or gain.dtype != torch.float32 or tuple(gain.shape) != (m, k):
        raise ValueError("deblur_frames: gain must be (%d, %d) float32, got %s %s" % (m, k, getattr(gain, "dtype", type(gain)), tuple(getattr(gain, "shape", ()))))
    radius, s = _check_deblur((k - 1) // 2, sensitivity, "deblur_frames")
    if h < 2 or w < 2:
        raise ValueError("deblur_frames: frames must be at least 2 x 2 (the bilinear taps), got %d x %d" % (w, h))
    if not (frames.is_cuda and maps.is_cuda and gain.is_cuda):
        raise ValueError("deblur_frames: frames, maps and gain must be on the device (there is no CPU path)")
    if out is None:
        out = torch.empty((m,) + tuple(frames.shape[1:]), dtype=frames.dtype, device=frames.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != frames.dtype or tuple(out.shape) != (m,) + tuple(frames.shape[1:]) or not out.is_cuda
          or not out.is_contiguous()):
        raise ValueError("deblur_frames: out must be a contiguous %s tensor %s on the device" % (frames.dtype, (m,) + tuple(frames.shape[1:])))
    frames, maps, gain = frames.contiguous(), maps.contiguous(), gain.contiguous()
    head = (A.ptr(frames), A.ptr(maps), A.ptr(gain), A.ptr(out), n, start, stop, radius)
    if fmt.hwc:
        A.check(A.lib().pws_deblur_u8(*head, h, w, s, A.current_stream()), "pws_deblur_u8")
    elif fmt.dtype == torch.uint8:
        A.check(A.lib().pws_deblur_plane_u8(*head, frames.shape[1], h, w, s, A.current_stream()), "pws_deblur_plane_u8")
    else:
        A.check(A.lib().pws_deblur_plane_u16(*head, frames.shape[1], h, w, fmt.layout, s, A.current_stream()), "pws_deblur_plane_u16")
    return out


def _zoom_windows(windows, n, frame_hw, what="zoom_fields"):
    """``windows`` -- one (x0, x1, y0, y1) or (n, 4) of them, a sequence or a tensor on either side -- as n tuples of floats; ValueError unless
    every one satisfies 0 <= x0 < x1 <= W0 and 0 <= y0 < y1 <= H0 (source-pixel EDGE coordinates: pixel k covers [k, k + 1))."""
    h0, w0 = int(frame_hw[0]), int(frame_hw[1])
    if isinstance(windows, torch.Tensor):
        windows = windows.detach().to("cpu", torch.float64).tolist()
    try:
        windows = list(windows)
        if len(windows) == 4 and not any(hasattr(v, "__len__") for v in windows):
            windows = [windows] * n
        windows = [tuple(float(v) for v in row) for row in windows]
    except (TypeError, ValueError):
        raise ValueError("%s: windows must be (x0, x1, y0, y1) or (T, 4) of them" % what) from None
    if len(windows) != n or any(len(row) != 4 for row in windows):
        raise ValueError("%s: windows must be one (x0, x1, y0, y1) or one per frame (%d, 4)" % (what, n))
    for t, (x0, x1, y0, y1) in enumerate(windows):
        if not (0 <= x0 < x1 <= w0 and 0 <= y0 < y1 <= h0):   # (False for NaN)
            raise ValueError("%s: window %d x [%g, %g) y [%g, %g) does not lie inside the %d x %d frame" % (what, t, x0, x1, y0, y1, w0, h0))
    return windows


def zoom_coefficients(windows, frame_hw, field_hw):
    """The (Ax, Bx, Ay, By) of ``pws_field_zoom`` for checked windows (``_zoom_windows``), in float64 on the host, rounded once to float32:
    (T, 4) float32 in pinned host memory.  Node j of the field stands for output pixel x = j (W0-1)/(fw-1) under the warps' align_corners=True
    resize; its centre x + 0.5 maps to x0 + (x + 0.5) Bx in the window, Bx = (x1 - x0) / W0, whose pixel coordinate, on the field's scale,
    is Bx j + Ax with Ax = (x0 + 0.5 Bx - 0.5) (fw-1)/(W0-1).  The whole frame gives exactly (0, 1, 0, 1)."""
    h0, w0 = int(frame_hw[0]), int(frame_hw[1])
    fh, fw = int(field_hw[0]), int(field_hw[1])
    if h0 < 2 or w0 < 2:
        raise ValueError("zoom_fields: the frame must be at least 2 x 2 pixels, got %d x %d" % (w0, h0))
    rows = []
    for x0, x1, y0, y1 in windows:
        bx, by = (x1 - x0) / w0, (y1 - y0) / h0
        rows.append([(x0 + 0.5 * bx - 0.5) * (fw - 1) / (w0 - 1), bx, (y0 + 0.5 * by - 0.5) * (fh - 1) / (h0 - 1), by])
    coef = torch.tensor(rows, dtype=torch.float64).reshape(len(rows), 4).to(torch.float32)
    return coef.pin_memory() if torch.cuda.is_available() else coef


def _field_operands(what, field, operands=(), name="field"):
    """ValueError unless every (name, tensor, dtype) of ``operands`` is a tensor of that dtype on the device and ``field`` is (T, fh, fw, 2)
    with at least 2 x 2 nodes: the first checks of every field operator, in this order."""
    for oname, t, dtype in operands:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
            raise ValueError("%s: %s must be a %s tensor on the device, got %s" % (
                what, oname, dtype, "%s on %s" % (t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t)))
    if field.dim() != 4 or field.shape[3] != 2 or field.shape[1] < 2 or field.shape[2] < 2:
        raise ValueError("%s: %s must be (T, fh, fw, 2) with fh, fw >= 2, got %s" % (what, name, tuple(field.shape),))


def _field_out(what, field, out, stats, *dtypes):
    """``out`` checked against ``field`` (ValueError), or allocated, and -- ``stats`` -- one (T,) device tensor per dtype, None otherwise."""
    if out is None:
        out = torch.empty(field.shape, device=field.device, dtype=torch.float32)
    elif tuple(out.shape) != tuple(field.shape) or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous %s float32 tensor" % (what, tuple(field.shape),))
    return [out] + [torch.empty((field.shape[0],), device=field.device, dtype=dt) if stats else None for dt in dtypes]


def _field_zoom(field, coef, frame_hw, align_corners, mode, out, uncovered):
    """pws_field_zoom on device tensors: ``coef`` (T, 4) float32, ``uncovered`` (T,) int32 or None."""
    A.check(A.lib().pws_field_zoom(A.ptr(field), field.shape[0], field.shape[1], field.shape[2], A.ptr(coef), A.ptr(out), int(frame_hw[0]),
                                   int(frame_hw[1]), _ac(align_corners), int(mode == "bicubic"), A.ptr(uncovered), A.current_stream()),
            "pws_field_zoom")
    return out


def zoom_fields(field, windows, frame_hw, align_corners=False, mode="bilinear", out=None, return_uncovered=False):
    """Zoom to fill, composed into the field: ``field`` (T, fh, fw, 2) as ``netG(window, False)`` returns it, resampled over ``windows`` --
    one (x0, x1, y0, y1) or (T, 4) of them, a sequence or a tensor, in source-pixel edge coordinates of the ``frame_hw`` = (H0, W0) frame
    (``auto_crop_window(..., output_hw=None)``'s convention: pixel k covers [k, k + 1), 0 <= x0 < x1 <= W0; fractional edges are fine,
    anything else is a ValueError).  A fused warp given the result produces the window of the frame it would have produced from ``field``,
    enlarged to the full frame, in its single resampling pass: node j samples the field at Bx j + Ax (``zoom_coefficients``), clamped to the
    field, with the warps' own field interpolation.  The field's values are kept, only its domain changes; the whole frame returns the
    field bit for bit.  The result is the warp of the RESAMPLED field -- sampled at the field's nodes, interpolated linearly between them
    by the warp -- not the exact composition.  One launch (csrc/field_zoom.hip); ``out`` must not overlap ``field``.
    return_uncovered: also a (T,) int32 device tensor, the number of nodes of each output field whose source position lies outside
    ``[m, W0-1-m] x [m, H0-1-m]`` -- m = 0 for mode "bilinear", 1 for "bicubic": ``keep_borders_``' coverage rule at the field's nodes, with
    ``align_corners`` the warp's.  0 means no node of the frame samples outside the source."""
    if mode not in INTERPOLATIONS:
        raise ValueError("mode must be one of %s, got %r" % (INTERPOLATIONS, mode))
    A.require_cuda(field)
    _field_operands("zoom_fields", field)
    field = field.contiguous()
    n = field.shape[0]
    coef = zoom_coefficients(_zoom_windows(windows, n, frame_hw), frame_hw, field.shape[1:3]).to(field.device, non_blocking=True)
    A.require_cuda(out)
    out, unc = _field_out("zoom_fields", field, out, return_uncovered, torch.int32)
    _field_zoom(field, coef, frame_hw, align_corners, mode, out, unc)
    return (out, unc) if return_uncovered else out


def _field_compose(field, d, frame_hw, align_corners, mode, out, uncovered):
    """pws_field_compose on device tensors: ``d`` (T, 6) float64, ``uncovered`` (T,) int32 or None."""
    A.check(A.lib().pws_field_compose(A.ptr(field), field.shape[0], field.shape[1], field.shape[2], A.ptr(d), A.ptr(out), int(frame_hw[0]),
                                      int(frame_hw[1]), _ac(align_corners), int(mode == "bicubic"), A.ptr(uncovered), A.current_stream()),
            "pws_field_compose")
    return out


def _field_compose_rows(field, d, rates, r, frame_hw, align_corners, mode, out, uncovered):
    """pws_field_compose_rows on device tensors: ``rates`` (T, 2, 4) float64, ``r`` the readout share in [-1, 1]."""
    A.check(A.lib().pws_field_compose_rows(A.ptr(field), field.shape[0], field.shape[1], field.shape[2], A.ptr(d), A.ptr(rates), float(r), A.ptr(out),
                                           int(frame_hw[0]), int(frame_hw[1]), _ac(align_corners), int(mode == "bicubic"), A.ptr(uncovered),
                                           A.current_stream()), "pws_field_compose_rows")
    return out


def _check_rolling_shutter(r, what):
    """``rolling_shutter`` as a float in [-1, 1]; ValueError otherwise (NaN included)."""
    try:
        v = float(r)
    except (TypeError, ValueError):
        raise ValueError("%s: rolling_shutter must be a number in [-1, 1], got %r" % (what, r)) from None
    if not -1.0 <= v <= 1.0:
        raise ValueError("%s: rolling_shutter must lie in [-1, 1], got %r" % (what, r))
    return v


def compose_fields(field, d, frame_hw, align_corners=False, mode="bilinear", out=None, return_uncovered=False, rates=None, rolling_shutter=0.0):
    """A per-frame affine correction of the output frame, composed into the field: ``field`` (T, fh, fw, 2) as ``netG(window, False)``
    returns it, ``d`` (T, 6) float64 on the device -- D of frame t, row-major 2 x 3, in pixels of the ``frame_hw`` = (H0, W0) frame relative
    to its centre, as ``stream.smooth_path`` returns it: output position p shows what the uncorrected output shows at D p.  A fused warp
    given the result produces that frame in its single resampling pass: node (i, j) takes the field at D of its own frame pixel, with the
    warps' own field interpolation; outside the lattice the field is continued linearly, so an affine field composes exactly and the
    wedges the correction opens reach the warp as out-of-range coordinates.  A frame whose D is exactly (1, 0, 0, 0, 1, 0) is copied bit for
    bit; a node that D sends to a position that is not finite keeps its value.  As with ``zoom_fields`` the result is the warp of the
    RESAMPLED field, not the exact composition.  One launch (csrc/field_compose.hip; include/pwstable.h has the definition); ``out`` must
    not overlap ``field``.
    return_uncovered: also a (T,) int32 device tensor, ``zoom_fields``' count on the composed field (``align_corners`` and ``mode`` the warp's).
    rates, rolling_shutter: the rolling-shutter correction.  ``rolling_shutter`` = r in [-1, 1] is the share of the frame interval that the
    sensor's readout takes from the top row to the bottom row (negative: bottom to top), ``rates`` (T, 2, 4) float64 on the device the
    camera's forward and backward velocity per frame, as ``stream.shutter_rates`` returns it.  D p lies on a row exposed delta = r
    clamp((D p).y / (H0 - 1), -1/2, 1/2) of a frame interval away from the centre row; the velocity field there (forward rates for delta >= 0,
    backward otherwise) times delta is taken out of D p before the field is read (csrc/field_compose.hip, the kernel's second
    instantiation; include/pwstable.h pws_field_compose_rows has the definition and its approximations).  A frame is then copied only if
    its D is the identity and its rates are all zero.  ``rolling_shutter == 0.0`` or ``rates is None`` is the call without them, bit for
    bit.
    ValueError: shapes or dtypes other than these, a host tensor, a frame below 2 x 2 pixels, an unknown mode, rolling_shutter outside [-1, 1]."""
    if mode not in INTERPOLATIONS:
        raise ValueError("mode must be one of %s, got %r" % (INTERPOLATIONS, mode))
    r = _check_rolling_shutter(rolling_shutter, "compose_fields")
    rows = r != 0.0 and rates is not None
    _field_operands("compose_fields", field, (("field", field, torch.float32), ("d", d, torch.float64)) + (
        (("out", out, torch.float32),) if out is not None else ()) + ((("rates", rates, torch.float64),) if rows else ()))
    n = field.shape[0]
    if tuple(d.shape) != (n, 6):
        raise ValueError("compose_fields: d must be (%d, 6), got %s" % (n, tuple(d.shape)))
    if rows and tuple(rates.shape) != (n, 2, 4):
        raise ValueError("compose_fields: rates must be (%d, 2, 4), got %s" % (n, tuple(rates.shape)))
    h0, w0 = int(frame_hw[0]), int(frame_hw[1])
    if h0 < 2 or w0 < 2:
        raise ValueError("compose_fields: the frame must be at least 2 x 2 pixels, got %d x %d" % (w0, h0))
    field, d = field.contiguous(), d.contiguous()
    out, unc = _field_out("compose_fields", field, out, return_uncovered, torch.int32)
    if rows:
        _field_compose_rows(field, d, rates.contiguous(), r, (h0, w0), align_corners, mode, out, unc)
    else:
        _field_compose(field, d, (h0, w0), align_corners, mode, out, unc)
    return (out, unc) if return_uncovered else out


def _check_rigidity(rigidity, what):
    """``rigidity`` as a float in [0, 1]; ValueError otherwise (NaN included)."""
    try:
        r = float(rigidity)
    except (TypeError, ValueError):
        raise ValueError("%s: rigidity must be a number in [0, 1], got %r" % (what, rigidity)) from None
    if not 0.0 <= r <= 1.0:
        raise ValueError("%s: rigidity must lie in [0, 1], got %r" % (what, rigidity))
    return r


def _field_rigid(field, m, frame_hw, rigidity, out, residual, unfit):
    """pws_field_rigid on device tensors: ``m`` (T, 9) or (T, 3, 3) float64, ``residual`` (T,) float32 / ``unfit`` (T,) int32 or None."""
    A.check(A.lib().pws_field_rigid(A.ptr(field), field.shape[0], field.shape[1], field.shape[2], A.ptr(m), float(rigidity), int(frame_hw[0]),
                                    int(frame_hw[1]), A.ptr(out), A.ptr(residual), A.ptr(unfit), A.current_stream()), "pws_field_rigid")
    return out


def rigid_fields(field, m, frame_hw, rigidity=1.0, out=None, return_stats=False):
    """Rigid warp mode, composed into the field: ``field`` (T, fh, fw, 2) as ``netG(window, False)`` returns it, blended towards the
    homographies ``m`` -- (T, 3, 3) or (T, 9) float64 on the device, as ``stream.field_homography(field, frame_hw)`` returns them: M maps a
    field value to the output position u = 2x/W0 - 1, v = 2y/H0 - 1 of the ``frame_hw`` = (H0, W0) frame.  Node (i, j) stands for frame
    pixel x = j (W0-1)/(fw-1), y = i (H0-1)/(fh-1); P = M^-1 (u, v) is where the homography alone would have it sample, in float64, rounded
    once.  The node becomes P at ``rigidity`` 1 -- every frame is warped by its fitted homography: straight lines stay straight -- and
    F + rigidity (P - F) below it; 0 returns the field bit for bit (the statistics are still computed).  A frame whose M is not finite or not invertible, and a node on or beyond the
    homography's horizon, keep F bit for bit.  One element-wise launch (csrc/field_rigid.hip; include/pwstable.h has the full
    definition); ``out`` may be ``field`` itself.  Any frame size: the 600 x 300 minimum is the fit's, not this function's.
    return_stats: also residual (T,) float32 -- per frame, how far the field was from rigid: the largest |F - P| in source pixels -- and
    unfit (T,) int32, the number of nodes that kept F because no homography applied to them; both on the device.
    ValueError: shapes or dtypes other than these, a host tensor, rigidity outside [0, 1]."""
    r = _check_rigidity(rigidity, "rigid_fields")
    _field_operands("rigid_fields", field, (("field", field, torch.float32), ("m", m, torch.float64)) + (
        (("out", out, torch.float32),) if out is not None else ()))
    n = field.shape[0]
    if tuple(m.shape) not in ((n, 3, 3), (n, 9)):
        raise ValueError("rigid_fields: m must be (%d, 3, 3) or (%d, 9), got %s" % (n, n, tuple(m.shape)))
    h0, w0 = int(frame_hw[0]), int(frame_hw[1])
    if h0 < 1 or w0 < 1:
        raise ValueError("rigid_fields: bad frame size %d x %d" % (w0, h0))
    out, res, unfit = _field_out("rigid_fields", field, out, return_stats, torch.float32, torch.int32)
    if out.data_ptr() == field.data_ptr() and not field.is_contiguous():
        raise ValueError("rigid_fields: out=field needs a contiguous field")
    field, m = field.contiguous(), m.contiguous()
    _field_rigid(field, m, (h0, w0), r, out, res, unfit)
    return (out, res, unfit) if return_stats else out


WOBBLE_MAX_SIGMA = 5.0   # frames: R = ceil(3 sigma) <= 15, the generator's own window of +-15 frames at period 30
WOBBLE_SEGMENT = 32      # the kernel's time segment, in output frames (include/pwstable.h PWS_WOBBLE_SEGMENT)


def _check_wobble(sigma, what, zero_ok=False):
    """``wobble`` / ``sigma`` as a float in (0, 5] (or [0, 5]); ValueError otherwise (NaN included)."""
    try:
        s = float(sigma)
    except (TypeError, ValueError):
        raise ValueError("%s: the wobble filter's sigma must be a number of frames, got %r" % (what, sigma)) from None
    if not ((0.0 < s or (zero_ok and s == 0.0)) and s <= WOBBLE_MAX_SIGMA):
        raise ValueError("%s: the wobble filter's sigma must lie in %s0, %g] frames, got %r" % (what, "[" if zero_ok else "(", WOBBLE_MAX_SIGMA, sigma))
    return s


def _field_wobble(field, m, frame_hw, sigma, out, removed, unfit):
    """pws_field_wobble on device tensors, ONE scene: ``m`` (n, 9) or (n, 3, 3) float64, ``removed`` (n,) float32 / ``unfit`` (n,) int32 or None."""
    A.check(A.lib().pws_field_wobble(A.ptr(field), field.shape[0], field.shape[1], field.shape[2], A.ptr(m), float(sigma), int(frame_hw[0]),
                                     int(frame_hw[1]), A.ptr(out), A.ptr(removed), A.ptr(unfit), A.current_stream()), "pws_field_wobble")
    return out


def wobble_fields(field, m, frame_hw, sigma, scene_cuts=None, out=None, return_stats=False):
    """Wobble suppression: the non-rigid part of a clip's fields low-passed along time.  ``field`` (T, fh, fw, 2) as ``netG(window, False)``
    returns it, ``m`` (T, 3, 3) or (T, 9) float64 on the device, as ``stream.field_homography(field, frame_hw)`` returns them, ``frame_hw`` =
    (H0, W0), ``sigma`` in (0, 5] frames.  Per node, P is the position the frame's homography alone would have it sample (``rigid_fields``'
    P, FITTED frame and VALID node, word for word) and E = F - P the residual: parallax, lens correction -- and the frame-to-frame shimmer
    of a field that is regressed from each frame's own window.  The node becomes P + sum g_k E[t+k] / sum g_k with g_k = exp(-k^2 / (2
    sigma^2)), |k| <= ceil(3 sigma) <= 15, over the frames of its scene at which the node is usable (fitted frame, valid node, finite F):
    taps beyond the scene's ends or at unusable nodes drop out of both sums -- no reflection, no padding.  A node that is not usable keeps
    F bit for bit.  The rigid part is untouched: a field that is exactly its homography comes back to within P's rounding, a residual that
    does not change in time comes back to a few ulps.  The filter acts at fixed OUTPUT positions: a real, fast change of parallax is smoothed
    too.  ``scene_cuts``: sorted indices at which a new scene starts; taps never cross a cut.  One launch per scene, on slices
    (csrc/field_wobble.hip; include/pwstable.h has the full definition); fixed order, no floating-point atomics: the same bits on every
    run.  ``out`` must not overlap ``field`` (the kernel reads neighbouring frames).  Any frame size: the 600 x 300 minimum is the fit's.
    return_stats: also removed (T,) float32 -- per frame, the largest distance in source pixels by which the filter moved a node: the number
    to choose sigma by -- and unfit (T,) int32, the nodes that kept F because they were not usable; both on the device, no synchronisation.
    ValueError: shapes or dtypes other than these, a host tensor, sigma outside (0, 5], bad cuts, an ``out`` that overlaps ``field``."""
    s = _check_wobble(sigma, "wobble_fields")
    _field_operands("wobble_fields", field, (("field", field, torch.float32), ("m", m, torch.float64)) + (
        (("out", out, torch.float32),) if out is not None else ()))
    n = field.shape[0]
    if tuple(m.shape) not in ((n, 3, 3), (n, 9)):
        raise ValueError("wobble_fields: m must be (%d, 3, 3) or (%d, 9), got %s" % (n, n, tuple(m.shape)))
    h0, w0 = int(frame_hw[0]), int(frame_hw[1])
    if h0 < 1 or w0 < 1:
        raise ValueError("wobble_fields: bad frame size %d x %d" % (w0, h0))
    out, removed, unfit = _field_out("wobble_fields", field, out, return_stats, torch.float32, torch.int32)
    cuts = _cut_list(scene_cuts, n, "wobble_fields")
    field, m = field.contiguous(), m.contiguous().reshape(n, 9)
    nbytes = field.numel() * 4
    if n and out.data_ptr() < field.data_ptr() + nbytes and field.data_ptr() < out.data_ptr() + nbytes:
        raise ValueError("wobble_fields: out must not overlap field (the filter reads neighbouring frames: it cannot run in place)")
    for a, b in (_scenes(n, cuts) if n else []):
        _field_wobble(field[a:b], m[a:b], (h0, w0), s, out[a:b], removed[a:b] if return_stats else None, unfit[a:b] if return_stats else None)
    return (out, removed, unfit) if return_stats else out


def adam_step_(p, g, m, v, lr, beta1, beta2, eps, step):
    """In-place fused Adam on flat fp32 CUDA buffers; the hyper-parameters travel as doubles (pws_adam_step_d)."""
    A.require_cuda(p, g, m, v)
    A.check(A.lib().pws_adam_step_d(A.ptr(p), A.ptr(g), A.ptr(m), A.ptr(v), p.numel(), lr, beta1, beta2, eps, step,
                                    A.current_stream()), "pws_adam_step_d")
