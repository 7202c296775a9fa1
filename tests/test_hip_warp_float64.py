"""The fp32 warp family (csrc/grid_sample.hip) against float64, through the C ABI: grid_sample forward and backward, affine_grid and its
adjoint, the align_corners=True resize and its adjoint, the fused resize + warp -- every instantiation the entry points dispatch to,
the streaming (non-temporal) variants on both sides of their thresholds included.

Two instruments (tests/warp_ref64.py):

  EXACT cases.  Power-of-two planes, coordinates in multiples of 1/64, 8-bit frames, integer upstream gradients: every intermediate of
  every formulation fits an fp32 significand, fp32 and float64 compute the same numbers, and the bound is ZERO -- outputs are compared
  with == on whole tensors (so -0.0 equals 0.0, and a NaN left from the fill equals nothing).  tests/test_warp_ref64_cpu.py shows that
  torch's own fp32 operators meet that bound on every exact shape used here.

  GENERAL cases, by the rule of tests/test_hip_bn_float64.py and tests/test_hip_objective_float64.py: on every compared tensor

      kernel error  <=  4 x torch-fp32 error  +  4 fp32 ulps of the tensor's largest float64 magnitude          (max over the tensor)

  where the yardstick is torch's fp32 evaluation of the same operation on the same inputs on the CPU and both errors are measured
  against the float64 reference.  The builders keep every sample 0.1 px from a cell boundary, so no element is excluded anywhere.

Every output is filled with NaN before the call.  tests/test_warp_ref64_cpu.py recomputes, from the thresholds in the sources' text,
that every row of the tables below reaches the kernel its comment names.

In brackets in the tests' docstrings: the largest kernel error / torch-fp32 error measured on an MI355X over the cases of that test,
and the largest share of a bound used."""
import functools
import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_ref64 as W  # noqa: E402
from test_hip_objective_float64 import Figures  # noqa: E402  (the rule itself: FACTOR = 4, ULPS = 4)
from pwstablenet_amd.hipabi import Exp  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
KINDS = ("scatter", "smooth")

# ------------------------------------------------------------------------------------------------------------ case tables
# (a) exact grid_sample: (n, c, h, w, ho, wo, ac), the forward's claim, the kernel of the field-only backward
FWD4, FWD1, FIELD, GENERAL = "grid_sample_fwd2_kernel<4, false>", "grid_sample_fwd2_kernel<1, false>", "grid_sample_bwd_field_kernel<false>", "grid_sample_bwd_kernel"
EXACT_ROWS = [
    ((2, 3, 64, 64, 64, 64, 0), {"kernel": FWD4, "nb": 8, "mod8": 0, "ragged": False}, FIELD),                     # four pixels per lane
    ((5, 3, 32, 32, 36, 52, 0), {"kernel": FWD4, "nb": 10, "mod8": 2, "ragged": True}, FIELD),                     # 2340 groups, groups that cross row ends
    ((3, 1, 16, 32, 5, 7, 0), {"kernel": FWD1, "nb": 1, "mod8": 1, "ragged": True}, GENERAL),                      # ho * wo % 4 != 0: one pixel per lane
    ((2, 3, 65, 257, 64, 64, 1), {"kernel": FWD4, "nb": 8, "mod8": 0, "ragged": False}, FIELD),                    # align_corners=True
    ((2, 3, 65, 257, 5, 7, 1), {"kernel": FWD1, "nb": 1, "mod8": 1, "ragged": True}, GENERAL),                     # align_corners=True, one pixel per lane
    ((2, 3, 4, 2, 8, 8, 0), {"kernel": FWD4, "nb": 1, "mod8": 1, "ragged": True}, FIELD),                          # w = 2: narrowest plane of the paired loads, xs always 0
    ((2, 3, 8, 1, 4, 4, 0), {"kernel": "grid_sample_fwd_kernel<4>", "nb": 1, "mod8": 1, "ragged": True}, GENERAL),  # w = 1, four pixels per lane
    ((2, 3, 8, 1, 3, 3, 0), {"kernel": "grid_sample_fwd_kernel<1>", "nb": 1, "mod8": 1, "ragged": True}, GENERAL),  # w = 1, one pixel per lane
    ((2, 31, 8, 8, 16, 16, 0), {"kernel": FWD4, "nb": 1, "mod8": 1, "ragged": True}, FIELD),                       # many channels
]
BASE_ROW = EXACT_ROWS[0][0]
# pointers 8 bytes into their allocations (every float2 access stays naturally aligned): the 16-byte fallbacks of both entry points
UNALIGNED_CLAIM = {"fwd": FWD1, "bwd_field_only": GENERAL}
# the 64 x 64 outputs once more under the experiments: (row, forward under GS_ROWWIN, field-only backward under GS_BWD_GENERAL)
EXPERIMENT_ROWS = [(EXACT_ROWS[0][0], "grid_sample_fwd2_kernel<4, false, true>", GENERAL), (EXACT_ROWS[3][0], "grid_sample_fwd2_kernel<4, false, true>", GENERAL)]

# (b) streaming sizes: c = 3, 256 x 256, one set of buffers of STREAM_N frames, calls on prefixes
STREAM_N, STREAM_SHAPE = 123, (3, 256, 256)
STREAM_FWD = [(122, {"kernel": FWD4, "streaming": False, "nb": 7808, "mod8": 0, "ragged": False}),                          # last non-streaming forward
              (123, {"kernel": "grid_sample_fwd2_kernel<4, true>", "streaming": True, "nb": 7872, "mod8": 0, "ragged": False})]   # first streaming: what bench.py times
STREAM_BWD = [(97, {"kernel": FIELD, "streaming": False, "nb": 6208, "mod8": 0, "ragged": False}),                          # last non-streaming field gradient
              (98, {"kernel": "grid_sample_bwd_field_kernel<true>", "streaming": True, "nb": 6272, "mod8": 0, "ragged": False})]  # first streaming

# (c) general sizes (n, c, h, w, ho, wo): forward claim, field-only backward kernel
GENERAL_ROWS = [
    ((1, 3, 37, 53, 37, 53), FWD1, GENERAL),      # odd everything: one pixel per lane, general backward
    ((2, 1, 40, 52, 24, 36), FWD4, FIELD),        # output smaller than the source, one channel
    ((3, 3, 17, 33, 8, 10), FWD4, FIELD),         # 20 groups: a single ragged block
]
SOURCES = ("u8", "smooth")

# (d) fused resize + warp, c = 3: (n, field (fh, fw), frame (h, w), output 8 bytes in?), claim
NARROW, WIDE, ONE = "upsample_grid_sample_fwd_kernel<4, true, false>", "upsample_grid_sample_fwd_kernel<4, false, false>", "upsample_grid_sample_fwd_kernel<1, false, false>"
FUSED_ROWS = [
    ((2, (5, 331), (8, 992), False), {"kernel": NARROW, "three_rx": 0.998991}),      # tightest NARROW
    ((2, (16, 16), (12, 48), False), {"kernel": NARROW, "three_rx": 0.957447}),      # NARROW
    ((2, (16, 16), (12, 44), False), {"kernel": WIDE, "three_rx": 1.046512}),        # wide
    ((1, (16, 16), (9, 50), False), {"kernel": ONE, "three_rx": 0.918367}),          # w % 4 != 0: one pixel per lane
    ((2, (16, 16), (12, 48), True), {"kernel": ONE, "three_rx": 0.957447}),          # alignment fallback
]
FUSED_EXACT = ((2, (64, 64), (64, 64), False), {"kernel": WIDE, "three_rx": 3.0})   # rx = ry = 1: the resize is the identity
FUSED_720P = ((256, 256), (720, 1280))
FUSED_STREAM = [(11, {"kernel": NARROW, "streaming": False, "nb": 9900, "mod8": 4, "ragged": False}),                        # last non-streaming
                (12, {"kernel": "upsample_grid_sample_fwd_kernel<4, true, true>", "streaming": True, "nb": 10800, "mod8": 0, "ragged": False})]   # first streaming

# (e) resize (h, w) -> (ho, wo) and affine_grid (h, w, ac)
RESIZE_EXACT = [((5, 9), (9, 33)), ((17, 3), (65, 5)), ((9, 9), (5, 5)), ((4, 4), (4, 4)), ((3, 4), (1, 1))]
RESIZE_GENERAL = [(2, 2, (256, 256), (720, 1280)), (2, 3, (5, 7), (11, 9))]        # (n, c, source, output)
AFFINE_EXACT = [(3, 16, 32, 0), (3, 17, 33, 1)]                                   # (n, h, w, ac)
AFFINE_BWD_EXACT = AFFINE_EXACT + [(64, 256, 256, 0)]
AFFINE_GENERAL = [(3, 33, 65, 0), (3, 33, 65, 1)]


def _x(row):
    return "x".join(str(v) for v in row)


# ------------------------------------------------------------------------------------------------------------ helpers
def _nan(shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


def _same(got, want, what):
    """whole tensors, ==: a bound of zero"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = int((got != want.to(got.device)).sum())
    assert bad == 0, "%s: %d of %d elements differ from float64" % (what, bad, got.numel())


def _same_bits(a, b, what):
    assert bool(torch.isfinite(a).all()), (what, "not finite")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


def _fwd(hip, img, grid, out, ac, n=None):
    _, c, h, w = img.shape
    ho, wo = grid.shape[1], grid.shape[2]
    hip.check(hip.lib().pws_grid_sample_fwd(hip.ptr(img), hip.ptr(grid), hip.ptr(out), img.shape[0] if n is None else n, c, h, w, ho, wo, int(ac),
                                            hip.current_stream()), "pws_grid_sample_fwd")


def _bwd(hip, gout, img, grid, ginput, ggrid, ac, n=None):
    _, c, h, w = img.shape
    ho, wo = grid.shape[1], grid.shape[2]
    hip.check(hip.lib().pws_grid_sample_bwd(hip.ptr(gout), hip.ptr(img), hip.ptr(grid), hip.ptr(ginput), hip.ptr(ggrid), img.shape[0] if n is None else n,
                                            c, h, w, ho, wo, int(ac), hip.current_stream()), "pws_grid_sample_bwd")


def _fused(hip, img, field, out, ac, n=None):
    _, c, h, w = img.shape
    fh, fw = field.shape[1], field.shape[2]
    hip.check(hip.lib().pws_upsample_grid_sample_fwd(hip.ptr(img), hip.ptr(field), hip.ptr(out), img.shape[0] if n is None else n, c, h, w, fh, fw,
                                                     int(ac), hip.current_stream()), "pws_upsample_grid_sample_fwd")


@functools.lru_cache(maxsize=None)
def exact_case(row, kind):
    """inputs of one exact row on the device and its float64 forward and backward (as fp32: asserted representable)"""
    n, c, h, w, ho, wo, ac = row
    seed = 17 * h + 3 * wo + (1 if kind == "smooth" else 0)
    case = {"img": W.exact_frames((n, c, h, w), seed, DEV), "grid": W.exact_field(n, ho, wo, h, w, ac, kind, seed + 1, DEV),
            "gout": W.exact_grads((n, c, ho, wo), seed + 2, DEV)}
    case.update(W.grid_sample64(case["img"], case["grid"], case["gout"], ac, exact=True))
    return case


# ------------------------------------------------------------------------------------------------------------ (a) exact grid_sample
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", [r[0] for r in EXACT_ROWS], ids=_x)
def test_grid_sample_exact_equals_float64(hip, row, kind):
    """Forward, the general backward (frame and field gradient) and the field-only backward equal float64 in every element."""
    ac, e = row[6], exact_case(row, kind)
    out, gi, gg, gg2 = _nan(e["out"].shape), _nan(e["img"].shape), _nan(e["grid"].shape), _nan(e["grid"].shape)
    _fwd(hip, e["img"], e["grid"], out, ac)
    _bwd(hip, e["gout"], e["img"], e["grid"], gi, gg, ac)
    _bwd(hip, e["gout"], e["img"], e["grid"], None, gg2, ac)
    _same(out, e["out"], "out")
    _same(gi, e["ginput"], "ginput")
    _same(gg, e["ggrid"], "ggrid (general backward)")
    _same(gg2, e["ggrid"], "ggrid (field-only backward)")
    assert float(e["ggrid"].abs().max()) > 0 and float(e["ginput"].abs().max()) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_grid_sample_exact_alignment_fallbacks(hip, kind):
    """Field, output, upstream gradient and field gradient 8 bytes into their allocations: the one-pixel forward and the general backward
    take over and give the same values."""
    ac, e = BASE_ROW[6], exact_case(BASE_ROW, kind)
    grid, gout = W.offset8(e["grid"].shape, DEV, e["grid"]), W.offset8(e["gout"].shape, DEV, e["gout"])
    out, gg = W.offset8(e["out"].shape, DEV, NAN), W.offset8(e["grid"].shape, DEV, NAN)
    _fwd(hip, e["img"], grid, out, ac)
    _bwd(hip, gout, e["img"], grid, None, gg, ac)
    _same(out, e["out"], "out")
    _same(gg, e["ggrid"], "ggrid")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", [r[0] for r in EXPERIMENT_ROWS], ids=_x)
def test_grid_sample_exact_under_experiments(hip, row, kind):
    """The field-only gradient through the general kernel (Exp.GS_BWD_GENERAL) and the row-window forward (Exp.GS_ROWWIN), whose fast path
    the smooth field takes: still float64."""
    ac, e = row[6], exact_case(row, kind)
    out, gg = _nan(e["out"].shape), _nan(e["grid"].shape)
    with hip.experiment(Exp.GS_ROWWIN):
        _fwd(hip, e["img"], e["grid"], out, ac)
    with hip.experiment(Exp.GS_BWD_GENERAL):
        _bwd(hip, e["gout"], e["img"], e["grid"], None, gg, ac)
    _same(out, e["out"], "out under GS_ROWWIN")
    _same(gg, e["ggrid"], "ggrid under GS_BWD_GENERAL")


@pytest.mark.parametrize("wrt", ["frame", "field", "both"])
def test_functional_grid_sample_autograd_exact(hip, wrt):
    """pwstablenet_amd.functional.grid_sample under autograd: a gradient for the frame only, for the field only, for both."""
    from pwstablenet_amd import functional as PF
    ac, e = BASE_ROW[6], exact_case(BASE_ROW, "scatter")
    img = e["img"].clone().requires_grad_(wrt in ("frame", "both"))
    grid = e["grid"].clone().requires_grad_(wrt in ("field", "both"))
    out = PF.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=bool(ac))
    out.backward(e["gout"])
    _same(out.detach(), e["out"], "out")
    if img.requires_grad:
        _same(img.grad, e["ginput"], "ginput")
    else:
        assert img.grad is None
    if grid.requires_grad:
        _same(grid.grad, e["ggrid"], "ggrid")
    else:
        assert grid.grad is None


# ------------------------------------------------------------------------------------------------------------ (b) streaming sizes
@functools.lru_cache(maxsize=1)
def stream_case():
    """123 frames of 3 x 256 x 256 built on the device (scatter on the first 62 samples, smooth on the rest) and their float64 forward
    and backward, computed once in chunks of 8 samples.  fp32 buffers and references together: 0.8 GB."""
    c, h, w = STREAM_SHAPE
    n, first = STREAM_N, (STREAM_N + 1) // 2
    case = {"img": W.exact_frames((n, c, h, w), 5, DEV), "gout": W.exact_grads((n, c, h, w), 6, DEV),
            "grid": torch.cat([W.exact_field(first, h, w, h, w, 0, "scatter", 7, DEV), W.exact_field(n - first, h, w, h, w, 0, "smooth", 8, DEV)])}
    case.update(W.grid_sample64(case["img"], case["grid"], case["gout"], 0, exact=True, chunk=8))
    return case


def _prefix_untouched(t, n):
    assert bool(torch.isnan(t[n:]).all()), "written past the %d samples of the call" % n


@pytest.mark.parametrize("n", [r[0] for r in STREAM_FWD])
def test_streaming_forward_equals_float64(hip, n):
    """n = 122: the last launch with plain loads and stores; n = 123: grid_sample_fwd2_kernel<4, true>, the kernel the benchmark times."""
    s = stream_case()
    out = _nan(s["out"].shape)
    _fwd(hip, s["img"], s["grid"], out, 0, n)
    _same(out[:n], s["out"][:n], "out")
    _prefix_untouched(out, n)


@pytest.mark.parametrize("n", [r[0] for r in STREAM_BWD])
def test_streaming_field_gradient_equals_float64(hip, n):
    """n = 97: grid_sample_bwd_field_kernel<false>; n = 98: <true>."""
    s = stream_case()
    gg = _nan(s["grid"].shape)
    _bwd(hip, s["gout"], s["img"], s["grid"], None, gg, 0, n)
    _same(gg[:n], s["ggrid"][:n], "ggrid")
    _prefix_untouched(gg, n)


def test_streaming_equals_plain_variants_bit_for_bit(hip):
    """n = 123 forward and n = 98 field gradient once more under Exp.GS_BWD_GENERAL, which is never non-temporal: float64 again, and the
    same bits as the streaming launches."""
    s = stream_case()
    nf, nb = STREAM_FWD[1][0], STREAM_BWD[1][0]
    out, gg, out_x, gg_x = _nan(s["out"].shape), _nan(s["grid"].shape), _nan(s["out"].shape), _nan(s["grid"].shape)
    _fwd(hip, s["img"], s["grid"], out, 0, nf)
    _bwd(hip, s["gout"], s["img"], s["grid"], None, gg, 0, nb)
    with hip.experiment(Exp.GS_BWD_GENERAL):
        _fwd(hip, s["img"], s["grid"], out_x, 0, nf)
        _bwd(hip, s["gout"], s["img"], s["grid"], None, gg_x, 0, nb)
    _same(out_x[:nf], s["out"][:nf], "out under GS_BWD_GENERAL")
    _same(gg_x[:nb], s["ggrid"][:nb], "ggrid under GS_BWD_GENERAL")
    _same_bits(out[:nf], out_x[:nf], "forward: streaming vs plain")
    _same_bits(gg[:nb], gg_x[:nb], "field gradient: streaming vs general")


def test_streaming_size_general_backward_equals_float64(hip):
    """The general backward with both gradients at n = 123: 8 million lanes, 97 million atomics."""
    s = stream_case()
    gi, gg = _nan(s["img"].shape), _nan(s["grid"].shape)
    _bwd(hip, s["gout"], s["img"], s["grid"], gi, gg, 0)
    _same(gi, s["ginput"], "ginput")
    _same(gg, s["ggrid"], "ggrid")


# ------------------------------------------------------------------------------------------------------------ (c) general sizes
def _general_inputs(row, ac, source):
    n, c, h, w, ho, wo = row
    seed = 100 + h + 7 * ac
    gen = torch.Generator().manual_seed(seed)
    img = W.exact_frames((n, c, h, w), seed) if source == "u8" else W.smooth_frames255(n, c, h, w, seed)
    return img, W.general_field(n, ho, wo, h, w, ac, seed), torch.randn((n, c, ho, wo), generator=gen)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("row", [r[0] for r in GENERAL_ROWS], ids=_x)
def test_grid_sample_general_vs_float64(hip, row, ac, source):
    """Sizes that cannot be exact, randn upstream gradients, uniform random 8-bit frames and smooth synth.make_frames frames: out, ginput
    and ggrid of the general backward, ggrid of the field-only backward, by the rule.
    [out 1.00, ginput 1.12, ggrid 1.00 from either backward kernel; largest share of a bound: out 0.24, ginput 0.27, ggrid 0.23]"""
    img, grid, gout = _general_inputs(row, ac, source)
    d_img, d_grid, d_gout = img.to(DEV), grid.to(DEV), gout.to(DEV)
    ref, t32 = W.grid_sample64(d_img, d_grid, d_gout, ac), W.grid_sample32(img, grid, gout, ac)
    out, gi, gg, gg2 = _nan(ref["out"].shape), _nan(img.shape), _nan(grid.shape), _nan(grid.shape)
    _fwd(hip, d_img, d_grid, out, ac)
    _bwd(hip, d_gout, d_img, d_grid, gi, gg, ac)
    _bwd(hip, d_gout, d_img, d_grid, None, gg2, ac)
    fig = Figures("grid_sample %s ac=%d %s:" % (_x(row), ac, source))
    fig.judge("out", out, ref["out"], t32["out"])
    fig.judge("ginput", gi, ref["ginput"], t32["ginput"])
    fig.judge("ggrid", gg, ref["ggrid"], t32["ggrid"])
    fig.judge("ggrid-only", gg2, ref["ggrid"], t32["ggrid"])
    fig.finish()


# ------------------------------------------------------------------------------------------------------------ (d) fused resize + warp
@pytest.mark.parametrize("kind", W.FUSED_KINDS)
@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("row", [r[0] for r in FUSED_ROWS], ids=lambda r: "%dx%s-to-%s%s" % (r[0], _x(r[1]), _x(r[2]), "-out+8" if r[3] else ""))
def test_fused_warp_vs_float64(hip, row, ac, kind):
    """pws_upsample_grid_sample_fwd on 8-bit frames against the float64 composition (resize of the field, then grid_sample), by the rule.
    [out 1.25 (16 x 16 -> 12 x 44, the wide path); largest share of a bound: 0.31]"""
    n, (fh, fw), (h, w), off = row
    seed = 7 * w + fh + ac
    img, field = W.exact_frames((n, 3, h, w), seed), W.fused_field(n, fh, fw, h, w, kind, seed + 1)
    d_img, d_field = img.to(DEV), field.to(DEV)
    out = W.offset8((n, 3, h, w), DEV, NAN) if off else _nan((n, 3, h, w))
    _fused(hip, d_img, d_field, out, ac)
    fig = Figures("fused %s ac=%d %s:" % (row, ac, kind))
    fig.judge("out", out, W.fused(d_img, d_field, ac), W.fused(img, field, ac, torch.float32))
    fig.finish()


def test_fused_warp_identity_resize_exact(hip):
    """A 64 x 64 field on 64 x 64 frames: rx = ry = 1, the resize is the identity, so with an exact scatter field the fused kernel equals
    float64 and equals pws_grid_sample_fwd bit for bit."""
    n, (fh, fw), (h, w), _ = FUSED_EXACT[0]
    img, field = W.exact_frames((n, 3, h, w), 31, DEV), W.exact_field(n, fh, fw, h, w, 0, "scatter", 32, DEV)
    out, plain = _nan((n, 3, h, w)), _nan((n, 3, h, w))
    _fused(hip, img, field, out, 0)
    _fwd(hip, img, field, plain, 0)
    _same(out, W.grid_sample64(img, field, None, 0, need=("out",), exact=True)["out"], "out")
    _same(out, W.fused(img, field, 0).float(), "out vs the float64 composition")
    _same_bits(out, plain, "fused vs pws_grid_sample_fwd")


@pytest.mark.parametrize("ac", [0, 1])
def test_fused_warp_720p_streaming(hip, ac):
    """12 frames of 720p on one set of buffers (the first half a stabiliser's field, the second half leaves the frame): n = 11 is the last
    launch with plain stores, n = 12 the first of upsample_grid_sample_fwd_kernel<4, true, true>.  n = 12 equals the run under
    Exp.GS_BWD_GENERAL (never non-temporal) in every bit, n = 11 equals the prefix of n = 12, and the first and the last sample meet the
    rule against float64.
    [first / last sample 1.12; largest share of a bound: 0.28]"""
    (fh, fw), (h, w) = FUSED_720P
    n = FUSED_STREAM[1][0]
    img = W.exact_frames((n, 3, h, w), 41 + ac, DEV)
    field = torch.cat([W.fused_field(n // 2, fh, fw, h, w, "stabiliser", 42), W.fused_field(n - n // 2, fh, fw, h, w, "leaves", 43)]).to(DEV)
    out12, out11, plain = _nan(img.shape), _nan(img.shape), _nan(img.shape)
    _fused(hip, img, field, out12, ac)
    _fused(hip, img, field, out11, ac, n - 1)
    with hip.experiment(Exp.GS_BWD_GENERAL):
        _fused(hip, img, field, plain, ac)
    _same_bits(out12, plain, "streaming vs plain")
    _same_bits(out11[:n - 1], out12[:n - 1], "n = 11 vs the prefix of n = 12")
    _prefix_untouched(out11, n - 1)
    fig = Figures("fused 720p ac=%d:" % ac)
    for i in (0, n - 1):
        fig.judge("sample %d" % i, out12[i:i + 1], W.fused(img[i:i + 1], field[i:i + 1], ac), W.fused(img[i:i + 1].cpu(), field[i:i + 1].cpu(), ac, torch.float32))
    fig.finish()


# ------------------------------------------------------------------------------------------------------------ (e) resize, affine_grid
def _resize_calls(hip, x, gout, ho, wo):
    n, c, h, w = x.shape
    L, st = hip.lib(), hip.current_stream()
    out, gin = _nan((n, c, ho, wo)), _nan(x.shape)
    hip.check(L.pws_upsample_bilinear_ac(hip.ptr(x), hip.ptr(out), n, c, h, w, ho, wo, st), "pws_upsample_bilinear_ac")
    hip.check(L.pws_upsample_bilinear_ac_bwd(hip.ptr(gout), hip.ptr(gin), n, c, h, w, ho, wo, st), "pws_upsample_bilinear_ac_bwd")
    return out, gin


@pytest.mark.parametrize("src,dst", RESIZE_EXACT, ids=lambda s: _x(s))
def test_resize_exact_equals_float64(hip, src, dst):
    """Power-of-two ratios and small integers: the resize and its adjoint equal float64."""
    (h, w), (ho, wo) = src, dst
    assert W.resize_is_exact(h, w, ho, wo)
    x, gout = W.exact_grads((2, 3, h, w), 50 + h, DEV), W.exact_grads((2, 3, ho, wo), 51 + h, DEV)
    ref, gref = W.resize(x, ho, wo, gout)
    assert bool((ref.float().double() == ref).all()) and bool((gref.float().double() == gref).all())
    out, gin = _resize_calls(hip, x, gout, ho, wo)
    _same(out, ref.float(), "out")
    _same(gin, gref.float(), "gin")


@pytest.mark.parametrize("n,c,src,dst", RESIZE_GENERAL, ids=lambda s: _x(s) if isinstance(s, tuple) else str(s))
def test_resize_general_vs_float64(hip, n, c, src, dst):
    """The field's own resize (256 x 256 -> 720 x 1280) and an odd small one, randn data, by the rule.
    [out 1.00, gin 1.07; largest share of a bound: out 0.25, gin 0.25]"""
    (h, w), (ho, wo) = src, dst
    gen = torch.Generator().manual_seed(60 + h)
    x, gout = torch.randn((n, c, h, w), generator=gen), torch.randn((n, c, ho, wo), generator=gen)
    ref, gref = W.resize(x.to(DEV), ho, wo, gout.to(DEV))
    t32, g32 = W.resize(x, ho, wo, gout, torch.float32)
    out, gin = _resize_calls(hip, x.to(DEV), gout.to(DEV), ho, wo)
    fig = Figures("resize %s -> %s:" % (src, dst))
    fig.judge("out", out, ref, t32)
    fig.judge("gin", gin, gref, g32)
    fig.finish()


def _affine_calls(hip, theta, ggrid, h, w, ac):
    n = theta.shape[0]
    L, st = hip.lib(), hip.current_stream()
    grid, gtheta = _nan((n, h, w, 2)), _nan((n, 6))
    hip.check(L.pws_affine_grid(hip.ptr(theta), hip.ptr(grid), n, h, w, ac, st), "pws_affine_grid")
    hip.check(L.pws_affine_grid_bwd(hip.ptr(ggrid), hip.ptr(gtheta), n, h, w, ac, st), "pws_affine_grid_bwd")
    return grid, gtheta


@pytest.mark.parametrize("n,h,w,ac", AFFINE_BWD_EXACT, ids=lambda v: str(v))
def test_affine_grid_exact_equals_float64(hip, n, h, w, ac):
    """Thetas in multiples of 1/64 on dyadic base coordinates: the grid equals float64; with integer upstream gradients the adjoint (summed
    in double by the kernel) equals the float64 sum rounded once to fp32."""
    theta, ggrid = W.exact_theta(n, 70 + h).to(DEV), W.exact_grads((n, h, w, 2), 71 + h, DEV)
    ref, gref = W.affine_grid64(theta, h, w, ac), W.affine_grid_bwd64(ggrid, ac)
    assert bool((ref.float().double() == ref).all())
    grid, gtheta = _affine_calls(hip, theta, ggrid, h, w, ac)
    _same(grid, ref.float(), "grid")
    _same(gtheta, gref.float(), "gtheta")


@pytest.mark.parametrize("n,h,w,ac", AFFINE_GENERAL, ids=lambda v: str(v))
def test_affine_grid_general_vs_float64(hip, n, h, w, ac):
    """33 x 65 (no base coordinate but 0 is dyadic), randn data, by the rule.
    [grid 1.25, gtheta 0.05 (the kernel sums in double); largest share of a bound: grid 0.15, gtheta 0.011]"""
    gen = torch.Generator().manual_seed(80 + ac)
    theta, ggrid = torch.randn((n, 6), generator=gen), torch.randn((n, h, w, 2), generator=gen)
    t32, g32 = W.affine_grid32(theta, h, w, ac, ggrid)
    grid, gtheta = _affine_calls(hip, theta.to(DEV), ggrid.to(DEV), h, w, ac)
    fig = Figures("affine_grid %dx%dx%d ac=%d:" % (n, h, w, ac))
    fig.judge("grid", grid, W.affine_grid64(theta, h, w, ac), t32)
    fig.judge("gtheta", gtheta, W.affine_grid_bwd64(ggrid, ac), g32)
    fig.finish()
