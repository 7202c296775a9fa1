"""The training objective's kernels (csrc/objective.hip) against float64 at the batch sizes the project trains at: every launch whose
grid is capped at kLossGrid workgroups on both sides of the cap, on walks that are ragged and whose block count is no multiple of the
8 XCDs, and every dispatch the wrappers take (one-pixel / four-pixel kernels, the lane hand-over of the temporal backward on rows
shorter than a wave, the general shape kernel).

The reference is tests/objective_ref64.py (float64 on the device; held to torch's float64 operators and to oracle/objective_ref.py
by tests/test_objective_ref64_cpu.py); it sees the fp32 values the kernels see.  Its builders make every compared element
well-conditioned (samples 0.1 px or more from a cell boundary, every L1 argument 0.04 or more from zero), so NO element is excluded
anywhere.  The yardstick is torch's own fp32 evaluation of the same operation on the same inputs, on the CPU, measured against the same
reference (the rule of tests/test_hip_bn_float64.py).  On every compared tensor

    kernel error  <=  4 x torch-fp32 error  +  4 fp32 ulps of the output's largest float64 magnitude          (max over the tensor)

and on the sums (one number's error is a noisy yardstick)

    |S_kernel - S64|  <=  4 x sum |per-term torch-fp32 error|  +  K * 2^-24 * S64

with K = the fp32 additions of one lane + 1, stated per kernel; the warp's L1 sum and the shape sums have bounds of their own (see
their tests).  tests/test_objective_ref64_cpu.py recomputes, from the constants in the sources' text, that every row of the tables
below reaches the path its comment names.

In brackets in the tests' docstrings: the largest kernel error / torch-fp32 error measured on an MI355X over the cases of that test,
and the largest share of a bound used."""
import ctypes
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objective_ref64 as R  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR, ULPS = 4.0, 4.0
EPS32 = 2.0 ** -24
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ------------------------------------------------------------------------------------------------------------ case tables
# Every shape is the smallest that reaches its path; the dicts are what tests/test_objective_ref64_cpu.py recomputes.
# warp_norm_fwd / warp_norm_bwd: (m, h, w), backward too?, forward claim, backward kernel
WARP_CASES = [
    ((32, 256, 256), True, {"nb": 2048, "capped": False, "mod8": 0, "ragged": False}, "warp_norm_bwd4_kernel"),   # last uncapped
    ((33, 256, 256), True, {"nb": 2112, "capped": True, "mod8": 0, "ragged": False}, "warp_norm_bwd4_kernel"),    # first capped
    ((64, 256, 256), False, {"nb": 4096, "capped": True, "mod8": 0, "ragged": False}, "warp_norm_bwd4_kernel"),   # configs[2]: forward and sum only
    # capped, nb % 8 = 5, ragged last block, odd row length, groups of 4 pixels crossing row ends
    ((3, 700, 1001), True, {"nb": 2053, "capped": True, "mod8": 5, "ragged": True}, "warp_norm_bwd4_kernel"),
    ((2, 3, 6), True, {"kernel": "refused"}, "warp_norm_bwd_kernel"),      # h * w % 4 != 0: the one-pixel backward; the forward refuses
    ((1, 2, 2), True, {"nb": 1, "capped": False, "mod8": 1, "ragged": True}, "warp_norm_bwd4_kernel"),            # w = 2: the narrowest row of the paired loads
]
WARP_SMOOTH = (2, 128, 128)     # one smooth synth.make_frames source (the other sources are uniform random 8-bit frames)
# (target, gextra, scale, accumulate)
WARP_VARIANTS = {"target + gextra": (True, True, None, 0), "target, scale 0.5": (True, False, 0.5, 0),
                 "gextra alone, accumulate": (False, True, 0.5, 1), "target + gextra, scale 0.5, accumulate": (True, True, 0.5, 1)}

# temporal_l1 fwd / bwd / bwd_det: (n, h, w), claim
TEMPORAL_CASES = [
    ((8, 256, 256), {"nb": 2048, "capped": False, "mod8": 0, "ragged": False, "g_pair": 1, "wave_spans_rows": False}),   # last uncapped
    ((9, 256, 256), {"nb": 2304, "capped": True, "mod8": 0, "ragged": False, "g_pair": 1, "wave_spans_rows": False}),    # first capped
    ((3, 419, 419), {"nb": 2058, "capped": True, "mod8": 2, "ragged": True, "g_pair": 0, "wave_spans_rows": True}),      # capped, ragged, no hand-over
    ((2, 48, 48), {"nb": 18, "capped": False, "mod8": 2, "ragged": False, "g_pair": 1, "wave_spans_rows": True}),        # hand-over meets row ends inside a wave
    ((3, 24, 24), {"nb": 7, "capped": False, "mod8": 7, "ragged": True, "g_pair": 0, "wave_spans_rows": True}),          # h*w % 64 == 0 but total % 256 != 0
]
TEMPORAL_TILED = [(2, 48, 48), (1, 70, 50)]       # EXP_TL1_TILED
KINDS = ["near identity", "rotation + zoom", "leaves the frame"]


def temporal_rows():
    """(n, h, w, kind, modes): the atomics' backward with every kind everywhere; the ordered gather walks a box per pixel, so above
    64 x 64 it runs with the near-identity theta only; the singular theta only at 16 x 16 and only for the gather; the tiles at their
    two shapes."""
    rows = []
    for (n, h, w), _ in TEMPORAL_CASES:
        for kind in KINDS:
            modes = ["fwd", "bwd"]
            if kind == "near identity" or max(h, w) <= 64:
                modes.append("det")
            if (n, h, w) in TEMPORAL_TILED:
                modes.append("tiled")
            rows.append((n, h, w, kind, tuple(modes)))
    rows.append((1, 70, 50, "rotation + zoom", ("fwd", "tiled")))
    rows.append((2, 16, 16, "degenerate", ("det",)))
    return rows


# field_smoothness: (m, h, w), one-pixel experiment?, claim
SMOOTH_CASES = [
    ((32, 256, 256), False, {"kernel": "field_smoothness4_kernel", "nb": 2048, "capped": False, "mod8": 0, "ragged": False}),   # last uncapped
    ((33, 256, 256), False, {"kernel": "field_smoothness4_kernel", "nb": 2112, "capped": True, "mod8": 0, "ragged": False}),    # first capped
    ((3, 699, 1004), False, {"kernel": "field_smoothness4_kernel", "nb": 2057, "capped": True, "mod8": 1, "ragged": True}),     # capped, ragged, nb4 % 8 = 1
    ((3, 700, 1001), False, {"kernel": "field_smoothness_kernel", "nb": 8212, "capped": True, "mod8": 4, "ragged": True}),      # one pixel per lane, capped fourfold
    ((1, 1, 4), False, {"kernel": "field_smoothness4_kernel", "nb": 1, "capped": False, "mod8": 1, "ragged": True}),            # no row below: dy == 0
    ((1, 5, 1), False, {"kernel": "field_smoothness_kernel", "nb": 1, "capped": False, "mod8": 1, "ragged": True}),             # no right-hand neighbour: dx == 0
    ((33, 256, 256), True, {"kernel": "field_smoothness_kernel", "nb": 8448, "capped": True, "mod8": 0, "ragged": False}),      # Exp.SMOOTH_ONE_PIXEL
]

# shape_loss: (m, size, block), general experiment?, claim
SHAPE_CASES = [
    ((32, 256, 16), False, {"kernel": "shape_loss16_kernel", "nb": 8192, "capped": False, "waves": 8192}),     # wave kernel, last uncapped
    ((33, 256, 16), False, {"kernel": "shape_loss16_kernel", "nb": 8448, "capped": True, "waves": 8192}),      # 8448 blocks on 8192 waves
    ((64, 256, 16), False, {"kernel": "shape_loss16_kernel", "nb": 16384, "capped": True, "waves": 8192}),     # configs[2]
    ((33, 256, 16), True, {"kernel": "shape_loss_kernel", "nb": 8448, "threads": 256, "live": 256}),          # Exp.SHAPE_GENERAL
    ((65, 64, 8), False, {"kernel": "shape_loss_kernel", "nb": 4160, "threads": 64, "live": 64}),             # general kernel
    ((65, 16, 4), False, {"kernel": "shape_loss_kernel", "nb": 1040, "threads": 64, "live": 16}),             # 16 live lanes of a 64-lane workgroup
]

# feature_loss fwd / bwd / bwd_det: (m, nf), field (h, w), claim
FEATURE_CASES = [
    ((64, 400), (256, 256), {"nb": 100, "ragged": False}),     # configs[2]
    ((65, 401), (60, 100), {"nb": 102, "ragged": True}),       # total not a multiple of 256, nf not a multiple of anything
    ((1, 1), (256, 256), {"nb": 1, "ragged": True}),           # a single point
]


# ------------------------------------------------------------------------------------------------------------ judging
def _x(shape):
    return "x".join(str(v) for v in shape)


def ulp32(x):
    return float(np.spacing(np.float32(x)))


class Figures:
    """Every (output, kernel error, torch-fp32 error, bound) of a case: printed, then asserted together."""

    def __init__(self, what):
        self.what, self.rows = what, []

    def judge(self, name, got, ref, t32):
        """a tensor: max error <= 4 x torch-fp32's max error + 4 ulps of the largest float64 magnitude"""
        assert bool(torch.isfinite(got).all()), (self.what, name, "not finite")
        ref = ref.double().to(got.device)
        ek, et = float((got.double() - ref).abs().max()), float((t32.to(got.device).double() - ref).abs().max())
        self.rows.append((name, ek, et, FACTOR * et + ULPS * ulp32(float(ref.abs().max()))))

    def judge_sum(self, name, got, ref, term_err, K):
        """a sum: error <= 4 x sum |per-term torch-fp32 error| + K * 2^-24 * S64"""
        self.rows.append((name, abs(float(got) - float(ref)), float(term_err), FACTOR * float(term_err) + K * EPS32 * abs(float(ref))))

    def judge_abs(self, name, err, bound):
        """a derived bound with no yardstick"""
        self.rows.append((name, float(err), 0.0, float(bound)))

    def finish(self):
        bad = []
        for name, ek, et, bound in self.rows:
            ratio = ek / et if et > 0 else float("inf") if ek > 0 else 0.0
            print("%s %-10s kernel %.3e torch32 %.3e ratio %8.3f of-bound %.3f%s" % (self.what, name, ek, et, ratio, ek / bound if bound > 0 else float(ek > 0),
                                                                                   "" if ek <= bound else "   <-- FAILS"))
            if not ek <= bound:
                bad.append((name, ek, et, bound))
        assert not bad, (self.what, bad)


def _slots(nq=1):
    return torch.zeros((nq, 64), device=DEV, dtype=torch.float64)


def _slot(slots, q):
    return ctypes.c_void_p(slots.data_ptr() + q * 64 * 8)


def _f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------ warp + L1
@functools.lru_cache(maxsize=1)
def warp_case(m, h, w, source="u8"):
    """The inputs of one shape, its float64 forward (computed once, shared by the forward test and every backward variant) and the frames
    as the product passes them: channel-range views of a 37-channel tensor (src_nstride = tgt_nstride = 37 h w)."""
    c = R.make_warp_case(m, h, w, seed=m + h, source=source, device=DEV)
    dev = torch.empty((m, 37, h, w), device=DEV)
    dev[:, 31:] = c["frames"].to(DEV)
    c["dev"], c["grid_dev"] = dev, c["grid"].to(DEV)
    return c


def _warp_fwd(hip, shape, source="u8"):
    m, h, w = shape
    c = warp_case(m, h, w, source)
    L, fr = hip.lib(), c["dev"]
    fake, slots = torch.full((m, 3, h, w), float("nan"), device=DEV), _slots()
    rc = L.pws_warp_norm_fwd(hip.ptr(fr[:, 31:]), fr.stride(0), hip.ptr(c["grid_dev"]), hip.ptr(fake), hip.ptr(fr[:, 34:]), fr.stride(0),
                             hip.ptr(slots), m, h, w, hip.current_stream())
    if R.dispatch_warp_fwd(m, h, w)["kernel"] == "refused":
        assert rc == -22, rc                       # PWS_EINVAL: the four-pixel forward takes h * w % 4 == 0 only
        torch.cuda.synchronize()
        assert bool(torch.isnan(fake).all()) and float(slots.abs().sum()) == 0.0
        return
    hip.check(rc, "pws_warp_norm_fwd")
    src = c["frames"][:, 0:3]
    t32 = F.grid_sample((src + 1) * 127.5, c["grid"], align_corners=False) / 127.5 - 1
    fig = Figures("warp fwd %s %s:" % (shape, source))
    fig.judge("fake", fake, c["fake64"], t32)
    own = float((fr[:, 34:37].double() - fake.double()).abs().sum())
    got = float(slots.sum())
    fig.judge_abs("l1 sum", abs(got - own), 16 * EPS32 * own)
    print("warp fwd %s: l1 %.9e, float64 of the kernel's own fake %.9e, float64 reference %.9e" % (shape, got, own, float(c["l1_64"])))
    fig.finish()


@pytest.mark.parametrize("shape", [r[0] for r in WARP_CASES], ids=_x)
def test_warp_norm_fwd_vs_float64(hip, shape):
    """fake within 4 x torch-fp32 error + 4 ulps on every element.  The L1 sum is compared with the float64 sum of |target - fake| over
    the kernel's OWN fake output: per lane the kernel takes 12 differences (one rounding each) and adds the 12 non-negative terms in
    fp32 (11 roundings, each at most 2^-24 of the partial sum, which never exceeds the lane's total); everything after the lane is
    double.  Each term is therefore off by at most (1 + 11) * 2^-24 of itself to first order: the bound is 16 * 2^-24 of the sum, with
    room for the second order.  A dropped or repeated block of the first capped launch moves the sum by 1 / 2112 = 5e-4 of it.
    (2, 3, 6): the forward refuses the shape (PWS_EINVAL) and writes nothing.
    [fake 1.00 on the four pixels of (1, 2, 2), 0.78 at the training batches (torch-fp32's error there is 3e-5: the fp32 pixel
    coordinate); largest share of a bound: fake 0.19, l1 sum 0.013 on four pixels and 1e-4 at the training batches]"""
    _warp_fwd(hip, shape)


def test_warp_norm_fwd_smooth_source_vs_float64(hip):
    """The same on one smooth synth.make_frames source (small image gradients: the error is the arithmetic's, not the coordinate's).
    [fake 0.50; largest share of a bound: fake 0.12, l1 sum 3e-4]"""
    _warp_fwd(hip, WARP_SMOOTH, "smooth")


def _warp_bwd(hip, shape, variant, source="u8"):
    m, h, w = shape
    use_t, use_g, scale, acc = WARP_VARIANTS[variant]
    c = warp_case(m, h, w, source)
    L, fr = hip.lib(), c["dev"]
    c_l1 = _f32(1.0 / (m * 3 * h * w))
    rs = np.random.RandomState(9)
    gextra = torch.from_numpy((rs.standard_normal((m, 3, h, w)) * c_l1).astype(np.float32)) if use_g else None
    base = torch.from_numpy((rs.standard_normal((m, h, w, 2)) * c_l1 * w).astype(np.float32)) if acc else None
    src, tgt = c["frames"][:, 0:3], c["frames"][:, 3:6]
    # kernel
    gg = base.to(DEV) if acc else torch.full((m, h, w, 2), float("nan"), device=DEV)
    sc = None if scale is None else torch.tensor([scale], device=DEV)
    ge = None if gextra is None else gextra.to(DEV)
    hip.check(L.pws_warp_norm_bwd(hip.ptr(fr[:, 31:]), fr.stride(0), hip.ptr(c["grid_dev"]), hip.ptr(fr[:, 34:]) if use_t else None, fr.stride(0),
                                  c_l1, hip.ptr(sc), hip.ptr(ge), hip.ptr(gg), acc, m, h, w, hip.current_stream()), "pws_warp_norm_bwd")
    # float64
    ref = R.warp_norm(fr[:, 31:34], c["grid_dev"], fr[:, 34:37] if use_t else None, c_l1, scale, ge, base.to(DEV) if acc else None)["ggrid"]
    # torch fp32 on the CPU
    g = c["grid"].clone().requires_grad_(True)
    fk = F.grid_sample((src + 1) * 127.5, g, align_corners=False) / 127.5 - 1
    loss = 0
    if use_t:
        loss = loss + (tgt - fk).abs().sum() * float(np.float32(c_l1) * np.float32(1.0 if scale is None else scale))
    if use_g:
        loss = loss + (fk * gextra).sum()
    loss.backward()
    t32 = g.grad + base if acc else g.grad
    fig = Figures("warp bwd %s %s [%s]:" % (shape, source, variant))
    fig.judge("ggrid", gg, ref, t32)
    return fig


@pytest.mark.parametrize("variant", list(WARP_VARIANTS))
@pytest.mark.parametrize("shape", [r[0] for r in WARP_CASES if r[1]], ids=_x)
def test_warp_norm_bwd_vs_float64(hip, shape, variant):
    """ggrid within 4 x torch-fp32 error + 4 ulps on every element (the field keeps every sample 0.1 px from a cell boundary and every
    L1 sign is decided): target with and without gextra, gextra alone (target NULL; scale then multiplies nothing), scale NULL and 0.5,
    accumulate 0 and 1 onto a random tensor.  (2, 3, 6) runs the one-pixel kernel, every other shape the four-pixel one.
    [ggrid 1.58 on the four pixels of (1, 2, 2), 1.01 at the training batches; largest share of a bound: 0.25]"""
    _warp_bwd(hip, shape, variant).finish()


def test_warp_norm_bwd_smooth_source_vs_float64(hip):
    """[ggrid 0.50; largest share of a bound: 0.12]"""
    _warp_bwd(hip, WARP_SMOOTH, "target + gextra, scale 0.5, accumulate", "smooth").finish()


# ------------------------------------------------------------------------------------------------------------ temporal L1
@pytest.mark.parametrize("n,h,w,kind,modes", temporal_rows(), ids=["%dx%dx%d-%s-%s" % (r[0], r[1], r[2], r[3], "+".join(r[4])) for r in temporal_rows()])
def test_temporal_l1_vs_float64(hip, n, h, w, kind, modes):
    """fwd: the sum, K = 4 (three fp32 additions per lane and block).  bwd (atomics; g_pair hand-over where the launch takes it), bwd_det
    (ordered gather) and the tiles of EXP_TL1_TILED: gfake2 = the caller's contents + the adjoint of the warp, within 4 x torch-fp32
    error + 4 ulps; gfake1 = the caller's contents - c * scale * sign(d), EQUAL BIT FOR BIT to the fp32 evaluation of that formula
    with the float64 signs (fake1 = fp32(warp64(fake2) + s u), |d| >= 0.04: every sign is decided).
    [sum 0.004 of its bound at most (the bound adds the terms' errors in absolute value, the kernel's error is their signed sum);
    gfake2: bwd 1.12, det 0.97, tiled 0.84 (the atomics' order moves the last digit run to run); largest share of a bound: 0.28]"""
    L, st = hip.lib(), hip.current_stream()
    c = R.make_temporal_case(n, h, w, kind, seed=n + h, device=DEV)
    f1, f2, th = c["fake1"].to(DEV), c["fake2"].to(DEV), c["theta"].to(DEV)
    cc, scale = _f32(10.0 / (n * 3 * h * w)), 2.0
    rs = np.random.RandomState(3)
    g1_0 = torch.from_numpy((rs.standard_normal((n, 3, h, w)) * cc).astype(np.float32))
    g2_0 = torch.from_numpy((rs.standard_normal((n, 3, h, w)) * cc).astype(np.float32))
    ref = R.temporal_l1(f1, f2, th, cc, scale, g1_0.to(DEV), g2_0.to(DEV))
    assert float(ref["d"].abs().min()) >= 0.04
    # torch fp32 on the CPU
    t2 = c["fake2"].clone().requires_grad_(True)
    grid = F.affine_grid(c["theta"].view(-1, 2, 3), (n, 3, h, w), align_corners=False)
    terms32 = (F.grid_sample(t2, grid, align_corners=False) - c["fake1"]).abs()
    coef = np.float32(cc) * np.float32(scale)
    (terms32.sum() * float(coef)).backward()
    t32_g2 = t2.grad + g2_0
    want_g1 = (g1_0 - torch.sign(ref["d"]).cpu().float() * coef).to(DEV)          # fp32: one product, one subtraction
    fig = Figures("temporal (%d, %d, %d) %s:" % (n, h, w, kind))
    sc = torch.tensor([scale], device=DEV)
    for mode in modes:
        if mode == "fwd":
            slots = _slots()
            hip.check(L.pws_temporal_l1_fwd(hip.ptr(f1), hip.ptr(f2), hip.ptr(th), hip.ptr(slots), n, h, w, st), "pws_temporal_l1_fwd")
            fig.judge_sum("sum", slots.sum(), ref["sum"], (terms32.detach().double() - ref["d"].abs().cpu()).abs().sum(), 4)
            continue
        g1, g2 = g1_0.to(DEV), g2_0.to(DEV)
        if mode == "det":
            scratch = torch.full((n, 3, h, w), float("nan"), device=DEV)
            hip.check(L.pws_temporal_l1_bwd_det(hip.ptr(f1), hip.ptr(f2), hip.ptr(th), cc, hip.ptr(sc), hip.ptr(g1), hip.ptr(g2), hip.ptr(scratch),
                                                n, h, w, st), "pws_temporal_l1_bwd_det")
        elif mode == "tiled":
            with hip.experiment(hip.Exp.TL1_TILED):
                hip.check(L.pws_temporal_l1_bwd(hip.ptr(f1), hip.ptr(f2), hip.ptr(th), cc, hip.ptr(sc), hip.ptr(g1), hip.ptr(g2), n, h, w, st), "tiled")
        else:
            hip.check(L.pws_temporal_l1_bwd(hip.ptr(f1), hip.ptr(f2), hip.ptr(th), cc, hip.ptr(sc), hip.ptr(g1), hip.ptr(g2), n, h, w, st),
                      "pws_temporal_l1_bwd")
        assert torch.equal(g1, want_g1), (mode, "gfake1 is not fp32(g - c * scale * sign(d))", float((g1 - want_g1).abs().max()))
        fig.judge("g2 " + mode, g2, ref["gfake2"], t32_g2)
    fig.finish()


def test_temporal_l1_bwd_scale_null(hip):
    """scale = NULL: the coefficient is c alone (gfake1 bit for bit, gfake2 within the bound).  [gfake2 0.86; share of the bound 0.21]"""
    L, st = hip.lib(), hip.current_stream()
    n, h, w = 2, 48, 48
    c = R.make_temporal_case(n, h, w, "rotation + zoom", seed=5, device=DEV)
    f1, f2, th = c["fake1"].to(DEV), c["fake2"].to(DEV), c["theta"].to(DEV)
    cc = _f32(0.37)
    ref = R.temporal_l1(f1, f2, th, cc)
    t2 = c["fake2"].clone().requires_grad_(True)
    grid = F.affine_grid(c["theta"].view(-1, 2, 3), (n, 3, h, w), align_corners=False)
    ((F.grid_sample(t2, grid, align_corners=False) - c["fake1"]).abs().sum() * cc).backward()
    g1, g2 = torch.zeros_like(f1), torch.zeros_like(f2)
    hip.check(L.pws_temporal_l1_bwd(hip.ptr(f1), hip.ptr(f2), hip.ptr(th), cc, None, hip.ptr(g1), hip.ptr(g2), n, h, w, st), "pws_temporal_l1_bwd")
    assert torch.equal(g1, (-torch.sign(ref["d"]).float() * np.float32(cc)))
    fig = Figures("temporal scale NULL:")
    fig.judge("g2", g2, ref["gfake2"], t2.grad)
    fig.finish()


# ------------------------------------------------------------------------------------------------------------ smoothness
@pytest.mark.parametrize("shape,one_pixel", [(r[0], r[1]) for r in SMOOTH_CASES], ids=[_x(r[0]) + ("-one-pixel" if r[1] else "") for r in SMOOTH_CASES])
def test_field_smoothness_vs_float64(hip, shape, one_pixel):
    """dx and dy sums.  Four pixels per lane: a lane adds the eight terms of a direction in fp32 (seven additions), K = 8; one pixel per
    lane: one addition, K = 2.  The per-term torch-fp32 error is the rounding of one subtraction, which the kernel makes too.  A field
    with one row (one column) has no neighbour below (to the right): that sum is exactly 0.
    [largest share of a bound: 0.10 on the four pixels of (1, 1, 4), below 0.001 at the capped shapes, where the bound adds the terms'
    errors in absolute value; a skipped block of the first capped launch is several hundred times the bound]"""
    m, h, w = shape
    L = hip.lib()
    gen = torch.Generator(device=DEV).manual_seed(m * 1000 + h)
    g = torch.randn((m, h, w, 2), device=DEV, generator=gen) * 0.3
    slots = _slots(2)
    if one_pixel:
        with hip.experiment(hip.Exp.SMOOTH_ONE_PIXEL):
            hip.check(L.pws_field_smoothness(hip.ptr(g), _slot(slots, 0), _slot(slots, 1), m, h, w, hip.current_stream()), "smooth1")
    else:
        hip.check(L.pws_field_smoothness(hip.ptr(g), _slot(slots, 0), _slot(slots, 1), m, h, w, hip.current_stream()), "smooth")
    got = slots.sum(1).cpu()
    ref = R.field_smoothness(g)
    gc = g.cpu()
    t32 = {"dx": (gc[:, :, :-1] - gc[:, :, 1:]).abs(), "dy": (gc[:, :-1] - gc[:, 1:]).abs()}
    K = 2 if R.dispatch_smooth(m, h, w, one_pixel)["kernel"] == "field_smoothness_kernel" else 8
    fig = Figures("smoothness %s%s:" % (shape, " one pixel" if one_pixel else ""))
    for k, name in enumerate(("dx", "dy")):
        fig.judge_sum(name, got[k], ref[name], (t32[name].double() - ref["terms_" + name].cpu()).abs().sum(), K)
    fig.finish()
    if h == 1:
        assert float(got[1]) == 0.0
    if w == 1:
        assert float(got[0]) == 0.0


# ------------------------------------------------------------------------------------------------------------ shape loss
@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import objective_ref
    return objective_ref


@pytest.mark.parametrize("shape,general", [(r[0], r[1]) for r in SHAPE_CASES], ids=[_x(r[0]) + ("-general" if r[1] else "") for r in SHAPE_CASES])
def test_shape_loss_vs_float64(hip, shape, general):
    """The kernels work in double on the fp32 residuals: the sum within 1e-12 relative of the reference (the explicit A (A^T A)^-1 A^T);
    gresid (fp32 of a double) within 4 x the error of oracle/objective_ref.py's float64 autograd rounded to fp32 + 4 ulps, with scale
    NULL and 2.0.  No residual |PB - B| is within 1e-9 of zero (asserted), so every sign is decided.
    [sum 1.5e-16 relative at most; gresid 1.00 (both are one rounding of the same double); largest share of a bound: 0.083]"""
    m, size, block = shape
    L, st = hip.lib(), hip.current_stream()
    resid = R.make_shape_resid(m, size, seed=m, block=block, device=DEV)
    d = resid.to(DEV)
    cc = 0.5
    r = resid.clone().requires_grad_(True)
    (_oracle().loss_shape(r, block, size) * cc).backward()
    fig = Figures("shape %s%s:" % (shape, " general" if general else ""))
    with hip.experiment(hip.Exp.SHAPE_GENERAL if general else 0):
        slots = _slots()
        hip.check(L.pws_shape_loss_fwd(hip.ptr(d), hip.ptr(slots), m, size, block, st), "pws_shape_loss_fwd")
        ref = R.shape_loss(d, block, cc)
        fig.judge_abs("sum", abs(float(slots.sum()) - float(ref["sum"])), 1e-12 * float(ref["sum"]))
        for scale in (None, 2.0):
            gr = torch.full_like(d, float("nan"))
            sc = None if scale is None else torch.tensor([scale], device=DEV)
            hip.check(L.pws_shape_loss_bwd(hip.ptr(d), cc, hip.ptr(sc), hip.ptr(gr), m, size, block, st), "pws_shape_loss_bwd")
            k = 1.0 if scale is None else scale
            fig.judge("gresid x%g" % k, gr, ref["gresid"] * k, r.grad * k)
    fig.finish()


# ------------------------------------------------------------------------------------------------------------ feature points
@pytest.mark.parametrize("shape,field", [(r[0], r[1]) for r in FEATURE_CASES], ids=[_x(r[0]) + "-on-" + _x(r[1]) for r in FEATURE_CASES])
def test_feature_loss_vs_float64(hip, shape, field):
    """fwd: the sum, K = 2 (dx * dx + dy * dy: one fp32 addition per lane).  bwd (atomics) and bwd_det (one lane per sample, in order):
    ggrid = the caller's contents - 2 c scale (unstable - field[pixel]) summed over the points of the pixel, within 4 x torch-fp32 error
    + 4 ulps, scale NULL and 2.0.  A quarter of each sample's points share their pixel with another point; sample 0 carries the edge
    coordinates -1.0, 0.999, -1.004 and -1.02 (the wrap of a negative index).
    [sum 0.076 of its bound at most; ggrid: bwd 1.49, det 2.25; largest share of a bound: 0.14]"""
    (m, nf), (h, w) = shape, field
    L, st = hip.lib(), hip.current_stream()
    rs = np.random.RandomState(m + nf)
    grid = torch.from_numpy(rs.uniform(-1, 1, (m, h, w, 2)).astype(np.float32))
    feats = R.make_features(m, nf, h, w, seed=m)
    base = torch.from_numpy((rs.standard_normal((m, h, w, 2)) * 1e-3).astype(np.float32))
    cc = _f32(1.0 / (nf * m))
    g, f = grid.to(DEV), feats.to(DEV)
    fig = Figures("feature %s on %s:" % (shape, field))
    # torch fp32 on the CPU: the same gather, the same terms
    q = R.feature_loss(grid, feats)["pixel"].reshape(-1)
    gt = grid.clone().requires_grad_(True)
    d32 = feats[..., 3:5].reshape(-1, 2) - gt.reshape(-1, 2)[q]
    terms32 = (d32 * d32).sum(-1)
    slots = _slots()
    hip.check(L.pws_feature_loss_fwd(hip.ptr(g), hip.ptr(f), hip.ptr(slots), m, nf, h, w, st), "pws_feature_loss_fwd")
    ref = R.feature_loss(g, f)
    fig.judge_sum("sum", slots.sum(), ref["sum"], (terms32.detach().double() - ref["terms"].reshape(-1).cpu()).abs().sum(), 2)
    terms32.sum().backward()
    for scale in (None, 2.0):
        coef = np.float32(cc) * np.float32(1.0 if scale is None else scale)
        ref_g = R.feature_loss(g, f, cc, scale, base.to(DEV))["ggrid"]
        t32 = base + gt.grad * coef
        sc = None if scale is None else torch.tensor([scale], device=DEV)
        for name, fn in (("bwd", L.pws_feature_loss_bwd), ("det", L.pws_feature_loss_bwd_det)):
            gg = base.to(DEV)
            hip.check(fn(hip.ptr(g), hip.ptr(f), cc, hip.ptr(sc), hip.ptr(gg), m, nf, h, w, st), "pws_feature_loss_" + name)
            fig.judge("ggrid %s x%g" % (name, 1.0 if scale is None else scale), gg, ref_g, t32)
    fig.finish()


# ------------------------------------------------------------------------------------------------------------ finalize
def test_objective_finalize_vs_float64(hip):
    """out[j] = sum_q coef[j, q] * (sum of quantity q's slots), in double, rounded once to fp32: within 1 ulp of the float64 result."""
    rs = np.random.RandomState(1)
    slots = torch.from_numpy(rs.uniform(0, 1e3, (16, 64)))
    coef = torch.from_numpy(rs.standard_normal((6, 16)) * (rs.uniform(0, 1, (6, 16)) < 0.5))
    out = torch.full((6,), float("nan"), device=DEV)
    sd, cd = slots.to(DEV), coef.to(DEV)
    hip.check(hip.lib().pws_objective_finalize(hip.ptr(sd), 16, hip.ptr(cd), 6, hip.ptr(out), hip.current_stream()), "pws_objective_finalize")
    want = R.finalize(slots, coef)
    for j in range(6):
        assert abs(float(out[j]) - float(want[j])) <= ulp32(abs(float(want[j]))), (j, float(out[j]), float(want[j]))


# ------------------------------------------------------------------------------------------------------------ the composite
def _smooth_field(n, size, seed, amp):
    spec = importlib.util.spec_from_file_location("mgo", os.path.join(GOLDEN, "make_golden_objective.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.smooth_field(n, size, seed, amp)


def test_composite_batch17_losses_vs_float64(hip):
    """StabObjective(batchSize=17) on m = 34 samples -- the smallest batch at which EVERY capped launch of the product is capped (warp,
    smoothness and shape above 32 samples, temporal above 8 items) -- on the smooth fields of make_golden_objective.smooth_field: the six
    reported losses against the float64 composition of tests/objective_ref64.py, and resid[2].grad against the shape reference.

    Each loss is a combination, with non-negative coefficients, of the kernels' sums, so its bound is the same combination of the sums'
    bounds: 4 x sum |per-term torch-fp32 error| + K * 2^-24 * S64 with the largest K of this file (16, the warp's L1), plus one fp32 ulp
    for the final conversion.  The per-term yardstick is oracle/objective_ref.py's composition in fp32 on the CPU (the warped frames,
    the temporal warp of those frames, the feature and smoothness terms).  The shape term is all double: 1e-12 relative + the ulp.

    The FIELD gradients are not compared here: on a smooth field the L1 signs cannot be decided by construction (fake is a function of
    the field, and the temporal term warps fake2 onto fake1), so a single flipped sign would need an exclusion.  The per-kernel tests
    above own the field gradients, on inputs whose signs are decided.
    [shares of the bounds: loss_g 0.04, loss_mse 0.006, loss_feature 0.02, loss_delta 0.01, loss_g2 0.009, loss_pixel 0.46 (its error is
    the final conversion to fp32); resid[2].grad 1.00 of the yardstick's error, 0.083 of its bound]"""
    from pwstablenet_amd import synth
    from pwstablenet_amd.objective import LOSS_NAMES, StabObjective
    n, size, nf, lamd = 17, 256, 400, 10.0
    m = 2 * n
    b = synth.make_train_batch(n, seed=41, size=size, number_feature=nf)
    imgs = torch.from_numpy(np.concatenate([b[0][:, 31:], b[3][:, 31:]], 0))            # (m, 6, size, size): unstable rgb, stable rgb
    norm = imgs.float() * (1. / 255) * 2 - 1
    feats = torch.from_numpy(np.concatenate([b[1], b[4]], 0)).float()
    adj = torch.from_numpy(b[6]).float().reshape(n, 6)
    grid_np, resid_np = _smooth_field(m, size, 42, 0.05)
    grids = [torch.from_numpy(grid_np) + np.float32(0.01 * k) for k in range(3)]
    resid = torch.from_numpy(resid_np)
    # the product
    d = norm.to(DEV)
    gd = [g.to(DEV).requires_grad_(True) for g in grids]
    rd = [resid.to(DEV).requires_grad_(True) for _ in range(3)]
    out = StabObjective(batchSize=n, number_feature=nf, lamd=lamd)(gd, rd, d[:, 0:3], d[:, 3:6], feats.to(DEV), adj.to(DEV))
    out.loss_g.backward()
    got = {k: float(out[k]) for k in LOSS_NAMES}
    # float64 and the fp32 yardstick, term by term
    cnt = float(n) * 3 * size * size
    S64 = {k: 0.0 for k in ("mse", "g2", "feature", "delta")}
    E32 = dict(S64)
    src, tgt, fd, th = d[:, 0:3], d[:, 3:6], feats.to(DEV), adj.to(DEV)
    q = R.feature_loss(grids[0], feats)["pixel"].reshape(-1)
    for nl in range(3):
        g64 = R.warp_norm(src, gd[nl].detach(), tgt)
        f32 = F.grid_sample((norm[:, 0:3] + 1) * 127.5, grids[nl], align_corners=False) / 127.5 - 1
        S64["mse"] += float(g64["l1"]) / cnt
        E32["mse"] += float(((norm[:, 3:6] - f32).abs().double() - g64["d"].abs().cpu()).abs().sum()) / cnt
        t64 = R.temporal_l1(g64["fake"][:n], g64["fake"][n:], th)
        o32 = F.grid_sample(f32[n:], F.affine_grid(adj.view(-1, 2, 3), (n, 3, size, size), align_corners=False), align_corners=False)
        S64["g2"] += float(t64["sum"]) / cnt
        E32["g2"] += float(((o32 - f32[:n]).abs().double() - t64["d"].abs().cpu()).abs().sum()) / cnt
        f64 = R.feature_loss(gd[nl].detach(), fd)
        d32 = feats[..., 3:5].reshape(-1, 2) - grids[nl].reshape(-1, 2)[q]
        S64["feature"] += float(f64["sum"]) / (nf * n)
        E32["feature"] += float(((d32 * d32).sum(-1).double() - f64["terms"].reshape(-1).cpu()).abs().sum()) / (nf * n)
        s64 = R.field_smoothness(gd[nl].detach())
        gc = grids[nl]
        cd = 0.5 / (float(n) * size * (size - 1) * 2)       # per branch (mean dx + mean dy) / 2, the two branches added
        S64["delta"] += (float(s64["dx"]) + float(s64["dy"])) * cd
        E32["delta"] += (float(((gc[:, :, :-1] - gc[:, :, 1:]).abs().double() - s64["terms_dx"].cpu()).abs().sum())
                         + float(((gc[:, :-1] - gc[:, 1:]).abs().double() - s64["terms_dy"].cpu()).abs().sum())) * cd
    sh = R.shape_loss(rd[2].detach(), 16, 1.0)
    want = {"loss_mse": S64["mse"], "loss_g2": S64["g2"], "loss_feature": S64["feature"], "loss_delta": S64["delta"], "loss_pixel": float(sh["sum"])}
    err = {"loss_mse": E32["mse"], "loss_g2": E32["g2"], "loss_feature": E32["feature"], "loss_delta": E32["delta"], "loss_pixel": 0.0}
    want["loss_g"] = want["loss_feature"] + want["loss_mse"] + want["loss_pixel"] + lamd * want["loss_g2"]
    err["loss_g"] = err["loss_feature"] + err["loss_mse"] + lamd * err["loss_g2"]
    fig = Figures("composite n = 17:")
    for k in LOSS_NAMES:
        derived = (1e-12 if k == "loss_pixel" else 16 * EPS32) * abs(want[k]) + ulp32(abs(want[k]))
        fig.rows.append((k, abs(got[k] - want[k]), err[k], FACTOR * err[k] + derived))
    fig.judge("resid grad", rd[2].grad, sh["gresid"], sh["gresid"].float())
    fig.finish()
    assert rd[0].grad is None and rd[1].grad is None
