"""float64 references, input builders and dispatch arithmetic of the fp32 warp family (csrc/grid_sample.hip: grid_sample forward and
backward, affine_grid and its adjoint, the align_corners=True resize and its adjoint, the fused resize + warp) -- TEST INFRASTRUCTURE
for tests/test_hip_warp_float64.py, held to torch's float64 operators by tests/test_warp_ref64_cpu.py.

References.  torch's own float64 F.grid_sample / F.interpolate with autograd, on whatever device the inputs live on, evaluated in chunks
of samples (a sample's result depends on nothing outside the sample).  affine_grid is restated ((2 j + 1) / size - 1, or
2 j / (size - 1) - 1, in double): torch builds its base grid from a linspace whose double rounding leaves 1e-16 of noise on values that
are dyadic rationals, which would hide the fact that the exact cases below are representable.

Exact builders.  For bilinear sampling there is an instrument sharper than any tolerance.  Take a source plane whose size is a power
of two (size - 1 for align_corners=True), sample coordinates whose fractions are multiples of 1/64, frames of 8-bit integers and
upstream gradients that are integers in [-8, 8].  Then every intermediate of every formulation is a dyadic rational that fits the 24
bits of an fp32 significand, so fp32 and float64 evaluate the SAME numbers whatever the order of operations:

    normalised coordinate  (2 px + 1) / W - 1          <= 6 + log2(W) fractional bits, magnitude < 16     (asserted by exact_field)
    pixel coordinate       one fmaf, result px          exact
    1-D weights            k / 64                       6 fractional bits;   2-D weights  <= 12 fractional bits
    value x weight         8 + 12                       <= 20 bits;  the blend of four is <= 255 with 12 fractional bits
    field gradient         per channel |go| * |(v01 - v00) wy0 + (v11 - v10) wy1| <= 8 * 255 with 6 fractional bits (17 bits);
                           a pixel's channel sum at c = 31 is < 2^16 with 6 fractional bits: <= 23 bits;  the final scale 0.5 * W
                           (0.5 * (W - 1)) is a power of two
    frame gradient         terms go * w: 12 fractional bits; a pixel's sum of |terms| stays under 2^10 (asserted on the
                           reference: grid_sample64(exact=True)), so every partial sum of every order is < 2^10 with 12 fractional bits: 22 bits

The tolerance of such a case is therefore not a number to tune: it is zero, and tests/test_warp_ref64_cpu.py shows that torch's fp32
operators meet it.  Any wrong tap, weight, border case, lane mapping or dropped store shows.

General builders keep every sample 0.1 px or more from a cell boundary (tests/objective_ref64.py make_warp_field, extended to an
output size of its own and to align_corners=True); the fused cases take a stabiliser's field (identity + ~5 % affine + a smooth
+-2 px residual) and one that leaves the frame on all four sides.

Dispatch arithmetic.  dispatch_fwd / dispatch_bwd / dispatch_fused return the kernel instantiation an entry point takes, from the
thresholds in the text of csrc/grid_sample.hip (the three `> 256e6` expressions, `3.f * rx < 0.999f`) and kXcds of common.h."""
import os
import re
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objective_ref64 as R  # noqa: E402
from objective_ref64 import ROOT  # noqa: E402

FRAC = 64                         # exact coordinates are multiples of 1 / FRAC
FRAC_K = (7, 57)                  # scatter fields: fraction k / 64, k in 7 .. 57
GRAD_INT = 8                      # upstream gradients: integers in [-8, 8]
SUM_ABS_LIMIT = 2.0 ** 10         # a frame-gradient pixel's sum of |terms|


def _d(t):
    return None if t is None else t.to(torch.float64)


# ------------------------------------------------------------------------------------------------------------ float64 references
def grid_sample64(img, grid, gout=None, ac=False, need=("out", "ginput", "ggrid"), chunk=8, exact=False):
    """torch's float64 F.grid_sample (bilinear, zeros) and its autograd on the inputs' device, `chunk` samples at a time.  Returns a dict
    of the tensors named in `need`.  exact=True: every result is asserted to be representable in fp32 and is returned AS fp32 (the same
    numbers in a third of the memory; comparing an fp32 kernel output with it by == is comparing with the float64 values), and with
    "ginput" the sum of |terms| of every frame-gradient pixel is asserted to stay under SUM_ABS_LIMIT."""
    n = img.shape[0]
    parts = {k: [] for k in need}
    for s in range(0, n, chunk):
        i = _d(img[s:s + chunk]).requires_grad_("ginput" in need)
        g = _d(grid[s:s + chunk]).requires_grad_("ggrid" in need)
        o = F.grid_sample(i, g, mode="bilinear", padding_mode="zeros", align_corners=bool(ac))
        res = {"out": o.detach()}
        wrt = [(name, t) for name, t in (("ginput", i), ("ggrid", g)) if t.requires_grad]
        if wrt:
            go = _d(gout[s:s + chunk])
            budget = exact and i.requires_grad
            for (name, _), grad in zip(wrt, torch.autograd.grad(o, [t for _, t in wrt], go, retain_graph=budget)):
                res[name] = grad
            if budget:
                worst = float(torch.autograd.grad(o, i, go.abs())[0].abs().max())
                assert worst < SUM_ABS_LIMIT, ("frame-gradient sum of |terms|", worst)
        for k in need:
            r = res[k]
            if exact:
                assert bool((r.float().double() == r).all()), (k, "float64 result not representable in fp32")
                r = r.float()
            parts[k].append(r)
    return {k: torch.cat(v) for k, v in parts.items()}


def grid_sample32(img, grid, gout=None, ac=False, need=("out", "ginput", "ggrid")):
    """torch's fp32 evaluation on the CPU: the yardstick of the 4 x + 4 ulps rule"""
    i = img.detach().cpu().float().clone().requires_grad_("ginput" in need)
    g = grid.detach().cpu().float().clone().requires_grad_("ggrid" in need)
    o = F.grid_sample(i, g, mode="bilinear", padding_mode="zeros", align_corners=bool(ac))
    if i.requires_grad or g.requires_grad:
        o.backward(gout.detach().cpu().float())
    res = {"out": o.detach(), "ginput": i.grad, "ggrid": g.grad}
    return {k: res[k] for k in need}


def base_coord64(size, ac, device="cpu"):
    j = torch.arange(size, dtype=torch.float64, device=device)
    if ac:
        return 2.0 * j / (size - 1) - 1.0 if size > 1 else torch.zeros_like(j)
    return (2.0 * j + 1.0) / size - 1.0


def affine_grid64(theta, h, w, ac=False):
    """F.affine_grid(theta, (n, C, h, w), align_corners=ac) in double from exact base coordinates: (n, h, w, 2)"""
    th = _d(theta).reshape(-1, 6)
    bx, by = base_coord64(w, ac, th.device).reshape(1, 1, w), base_coord64(h, ac, th.device).reshape(1, h, 1)
    c = [th[:, k].reshape(-1, 1, 1) for k in range(6)]
    return torch.stack([c[0] * bx + c[1] * by + c[2], c[3] * bx + c[4] * by + c[5]], -1)


def affine_grid_bwd64(ggrid, ac=False):
    """the adjoint: gtheta[n] = sum_{y, x} ggrid[n, y, x, :] (x) [x, y, 1]: (n, 6)"""
    g = _d(ggrid)
    n, h, w, _ = g.shape
    bx, by = base_coord64(w, ac, g.device).reshape(1, 1, w), base_coord64(h, ac, g.device).reshape(1, h, 1)
    cols = []
    for k in range(2):
        cols += [(g[..., k] * bx).sum((1, 2)), (g[..., k] * by).sum((1, 2)), g[..., k].sum((1, 2))]
    return torch.stack(cols, 1)


def affine_grid32(theta, h, w, ac=False, ggrid=None):
    """torch's fp32 F.affine_grid on the CPU, and with `ggrid` its autograd: (grid, gtheta (n, 6))"""
    th = theta.detach().cpu().float().reshape(-1, 2, 3).clone().requires_grad_(ggrid is not None)
    g = F.affine_grid(th, (th.shape[0], 1, h, w), align_corners=bool(ac))
    if ggrid is None:
        return g.detach(), None
    g.backward(ggrid.detach().cpu().float())
    return g.detach(), th.grad.reshape(-1, 6)


def resize(x, ho, wo, gout=None, dtype=torch.float64):
    """F.interpolate(x, (ho, wo), mode="bilinear", align_corners=True) and, with `gout`, its adjoint, in `dtype` on x's device"""
    i = x.detach().to(dtype).clone().requires_grad_(gout is not None)
    o = F.interpolate(i, size=(ho, wo), mode="bilinear", align_corners=True)
    if gout is None:
        return o.detach(), None
    o.backward(gout.detach().to(dtype))
    return o.detach(), i.grad


def fused(img, field, ac=False, dtype=torch.float64):
    """the fused warp as its composition: the field (n, fh, fw, 2) resized (as NCHW, align_corners=True) to the frame, then grid_sample"""
    h, w = img.shape[2], img.shape[3]
    up = F.interpolate(field.detach().to(dtype).permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    return F.grid_sample(img.detach().to(dtype), up, mode="bilinear", padding_mode="zeros", align_corners=bool(ac))


# ------------------------------------------------------------------------------------------------------------ exact builders
def _pow2(v):
    return v >= 1 and (v & (v - 1)) == 0


def exact_field(m, ho, wo, h, w, ac, kind, seed, device="cpu"):
    """(m, ho, wo, 2) fp32 field of an h x w source whose pixel coordinates are multiples of 1/64, built from PIXEL coordinates,
    normalised in double and asserted to survive the rounding to fp32 unchanged.
      "scatter": integer part uniform over [-3, size + 2] in both axes, fraction k / 64 with k in 7 .. 57; the last pixels of sample 0
                 sit on the frame's corners and edges and the first min(8, pixels / 4) pixels of the last sample lie 5 frame widths
                 outside, as make_warp_field places them;
      "smooth":  px = x + a[n, y], py = y + b[n, y] with a, b multiples of 1/64 in [-2, 2]: the four pixels of a lane read consecutive
                 columns of one row pair (a stabiliser's access pattern, the only one on which the row-window experiment runs fast).
    ac=False needs h and w to be powers of two, ac=True h - 1 and w - 1; other sizes are refused."""
    ok = (_pow2(h - 1) and _pow2(w - 1)) if ac else (_pow2(h) and _pow2(w))
    if not ok:
        raise ValueError("exact_field: %d x %d source with align_corners=%d is not exact" % (h, w, int(ac)))
    gen = torch.Generator(device=device).manual_seed(seed)

    def ri(lo, hi, shape):   # integers lo .. hi - 1 as double
        return torch.randint(lo, hi, shape, generator=gen, device=device).double()
    if kind == "scatter":
        px = ri(R.INT_LO, w + R.INT_PAST + 1, (m, ho, wo)) + ri(FRAC_K[0], FRAC_K[1] + 1, (m, ho, wo)) / FRAC
        py = ri(R.INT_LO, h + R.INT_PAST + 1, (m, ho, wo)) + ri(FRAC_K[0], FRAC_K[1] + 1, (m, ho, wo)) / FRAC
        far = min(R.FAR, ho * wo // 4)
        corners = [(-1, -1), (w - 1, h - 1), (0, 0), (-1, h - 1), (w - 1, -1), (0, -1)][:ho * wo - far]
        cx, cy = px[0].reshape(-1), py[0].reshape(-1)              # views
        for k, (x0, y0) in enumerate(corners):
            i = ho * wo - 1 - k
            cx[i], cy[i] = x0 + (cx[i] - torch.floor(cx[i])), y0 + (cy[i] - torch.floor(cy[i]))
        sgn = torch.where(torch.arange(far, device=device) % 2 == 0, -5.0, 6.0).double()
        fx, fy = px[m - 1].reshape(-1), py[m - 1].reshape(-1)      # views
        fx[:far] = sgn * w + ri(FRAC_K[0], FRAC_K[1] + 1, (far,)) / FRAC
        fy[far // 2:far] = sgn[far // 2:] * h + ri(FRAC_K[0], FRAC_K[1] + 1, (far - far // 2,)) / FRAC
    elif kind == "smooth":
        a, b = ri(-2 * FRAC, 2 * FRAC + 1, (m, ho, 1)) / FRAC, ri(-2 * FRAC, 2 * FRAC + 1, (m, ho, 1)) / FRAC
        px = torch.arange(wo, device=device).double().reshape(1, 1, wo) + a
        py = torch.arange(ho, device=device).double().reshape(1, ho, 1) + b + torch.zeros((m, ho, wo), dtype=torch.float64, device=device)
        px = px.expand(m, ho, wo)
    else:
        raise ValueError(kind)
    if ac:
        g = torch.stack([2.0 * px / (w - 1) - 1.0, 2.0 * py / (h - 1) - 1.0], -1)
    else:
        g = torch.stack([(2.0 * px + 1.0) / w - 1.0, (2.0 * py + 1.0) / h - 1.0], -1)
    g32 = g.float()
    assert bool((g32.double() == g).all()), "exact_field: the field is not representable in fp32"
    return g32.contiguous()


def exact_frames(shape, seed, device="cpu"):
    """randint(0, 256) as fp32"""
    gen = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(0, 256, shape, generator=gen, device=device).float()


def exact_grads(shape, seed, device="cpu", bound=GRAD_INT):
    """randint(-8, 9) as fp32"""
    gen = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(-bound, bound + 1, shape, generator=gen, device=device).float()


def exact_theta(n, seed):
    """(n, 6) multiples of 1/64 in [-2, 2]"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-2 * FRAC, 2 * FRAC + 1, (n, 6), generator=gen).float() / FRAC


def resize_is_exact(h, w, ho, wo):
    """(h - 1) / (ho - 1) and (w - 1) / (wo - 1) are powers of two (or the output size is 1): source indices and weights are dyadic"""
    def one(a, b):
        if b == 1 or a == 1:
            return True
        p, q = a - 1, b - 1
        return (p % q == 0 and _pow2(p // q)) or (q % p == 0 and _pow2(q // p))
    return one(h, ho) and one(w, wo)


# ------------------------------------------------------------------------------------------------------------ general builders
def general_field(m, ho, wo, h, w, ac, seed):
    """make_warp_field for an output size of its own and either coordinate convention: (m, ho, wo, 2) fp32 built from pixel coordinates of
    the h x w source -- integer part uniform over [-3, size + 2], fraction uniform over [0.1, 0.9] (0.1 px from every cell boundary; fp32
    coordinate rounding is ~W/2 * 2^-24 px), sample 0's last pixels on the corners and edges, the last sample's first pixels 5 frame
    widths outside -- normalised in double, then rounded to fp32."""
    rs = np.random.RandomState(seed)
    px = rs.randint(R.INT_LO, w + R.INT_PAST + 1, (m, ho, wo)) + rs.uniform(R.FRAC_LO, R.FRAC_HI, (m, ho, wo))
    py = rs.randint(R.INT_LO, h + R.INT_PAST + 1, (m, ho, wo)) + rs.uniform(R.FRAC_LO, R.FRAC_HI, (m, ho, wo))
    far = min(R.FAR, ho * wo // 4)
    corners = [(-1, -1), (w - 1, h - 1), (0, 0), (-1, h - 1), (w - 1, -1), (0, -1)][:ho * wo - far]
    cx, cy = px[0].reshape(-1), py[0].reshape(-1)
    for k, (x0, y0) in enumerate(corners):
        i = ho * wo - 1 - k
        cx[i], cy[i] = x0 + (cx[i] - np.floor(cx[i])), y0 + (cy[i] - np.floor(cy[i]))
    sgn = np.where(np.arange(far) % 2 == 0, -5.0, 6.0)
    fx, fy = px[m - 1].reshape(-1), py[m - 1].reshape(-1)
    fx[:far] = sgn * w + rs.uniform(R.FRAC_LO, R.FRAC_HI, far)
    fy[far // 2:far] = sgn[far // 2:] * h + rs.uniform(R.FRAC_LO, R.FRAC_HI, far - far // 2)
    if ac:
        g = np.stack([2.0 * px / (w - 1) - 1.0, 2.0 * py / (h - 1) - 1.0], -1)
    else:
        g = np.stack([(2.0 * px + 1.0) / w - 1.0, (2.0 * py + 1.0) / h - 1.0], -1)
    g = g.astype(np.float32)
    # the guarantee, on the fp32 field itself: un-normalised in double, no sample within 0.09 px of a cell boundary
    for k, size in ((0, w), (1, h)):
        p = (g[..., k].astype(np.float64) + 1.0) * 0.5 * (size - 1) if ac else ((g[..., k].astype(np.float64) + 1.0) * size - 1.0) * 0.5
        fr = p - np.floor(p)
        assert fr.min() > 0.09 and fr.max() < 0.91, (fr.min(), fr.max())
    return torch.from_numpy(g)


FUSED_KINDS = ("stabiliser", "leaves")


def fused_field(n, fh, fw, h, w, kind, seed):
    """(n, fh, fw, 2) fp32 field in normalised coordinates of an h x w frame.  "stabiliser": identity + ~5 % affine + a smooth residual of
    +-2 px.  "leaves": the same around a zoom-out (1.4 x and the residual's 4 / size) with a shear, so that the frame is left on all four sides
    (asserted)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, fh), np.linspace(-1, 1, fw), indexing="ij")
    out = np.empty((n, fh, fw, 2), np.float64)
    for i in range(n):
        base = np.array([1.4 + 4.0 / w, 0.1, 0.0, -0.1, 1.4 + 4.0 / h, 0.0]) if kind == "leaves" else np.array([1.0, 0, 0, 0, 1.0, 0])
        t = base + 0.05 * rs.uniform(-1, 1, 6)
        for k, size in ((0, w), (1, h)):
            fx, fy, ph = rs.uniform(0.5, 2.0), rs.uniform(0.5, 2.0), rs.uniform(0, 6.28)
            resid = (2.0 * 2.0 / size) * np.sin(np.pi * (fx * xx + fy * yy) + ph)     # +-2 px in normalised units
            out[i, :, :, k] = t[3 * k] * xx + t[3 * k + 1] * yy + t[3 * k + 2] + resid
        if kind == "leaves":
            assert out[i, :, 0, 0].max() < -1 and out[i, :, -1, 0].min() > 1 and out[i, 0, :, 1].max() < -1 and out[i, -1, :, 1].min() > 1
    return torch.from_numpy(out.astype(np.float32))


def smooth_frames255(n, c, h, w, seed):
    """synth.make_frames rounded to 8-bit values, 0 .. 255 as fp32"""
    from pwstablenet_amd import synth
    return torch.from_numpy(np.round(synth.make_frames(n, c, h, w, seed=seed)).astype(np.float32))


def offset8(shape, device, fill=None):
    """an fp32 tensor of `shape` whose storage begins 8 bytes into its allocation: 8-byte but not 16-byte aligned"""
    numel = int(np.prod(shape))
    flat = torch.empty(numel + 2, device=device, dtype=torch.float32)
    t = flat[2:].view(shape)
    assert t.data_ptr() % 16 == 8
    if fill is not None:
        t.copy_(fill) if isinstance(fill, torch.Tensor) else t.fill_(fill)
    return t


# ------------------------------------------------------------------------------------------------------------ dispatch arithmetic
def _exp_ids():
    from pwstablenet_amd.hipabi import Exp
    return {"general": int(Exp.GS_BWD_GENERAL), "cvt": int(Exp.U8_CVT_SHIFT), "rowwin": int(Exp.GS_ROWWIN)}


def source_constants():
    """The streaming thresholds of the three entry points (coefficient expression in c, bytes), the NARROW rule and kXcds, read from the
    sources' text"""
    with open(os.path.join(ROOT, "pwstablenet_amd/csrc/grid_sample.hip")) as f:
        text = f.read()
    with open(os.path.join(ROOT, "pwstablenet_amd/csrc/common.h")) as f:
        common = f.read()

    def body(name):
        mt = re.search(r'extern "C" int %s\(.*?\n}\n' % name, text, re.S)
        assert mt, name
        return mt.group(0)

    def threshold(name):
        found = re.findall(r"\(double\)total \* ([0-9.c+*() ]+?) > ([0-9.e]+)", body(name))
        assert len(found) == 1, (name, found)
        expr, limit = found[0]
        assert re.fullmatch(r"[0-9.c+*() ]+", expr)
        return expr, float(limit)
    narrow = set(re.findall(r"([0-9.]+)f \* rx < ([0-9.]+)f", body("pws_upsample_grid_sample_fwd")))
    assert len(narrow) == 1, narrow
    span, below = narrow.pop()
    xcds = re.search(r"constexpr\s+int\s+kXcds\s*=\s*(\d+)\s*;", common)
    assert xcds
    return {"fwd": threshold("pws_grid_sample_fwd"), "bwd": threshold("pws_grid_sample_bwd"), "fused": threshold("pws_upsample_grid_sample_fwd"),
            "narrow": (np.float32(span), np.float32(below)), "kXcds": int(xcds.group(1)), "exp": _exp_ids()}


def _streams(k, which, total, c):
    expr, limit = k[which]
    return float(total) * float(eval(expr, {"__builtins__": {}}, {"c": c})) > limit


def _walk(units, k):
    nb = -(-units // 256)
    return {"nb": nb, "mod8": nb % k["kXcds"], "ragged": units % 256 != 0}


def dispatch_fwd(n, c, h, w, ho, wo, aligned=True, exp=0, k=None):
    """pws_grid_sample_fwd: the kernel instantiation, pixels per lane, streaming, block count, nb % 8, ragged last block"""
    k = k or source_constants()
    e = k["exp"]
    total, four = n * ho * wo, (ho * wo) % 4 == 0 and aligned
    if four and w >= 2:
        nt = exp not in (e["general"], e["cvt"]) and _streams(k, "fwd", total, c)
        name = "grid_sample_fwd2_kernel<4, %s%s>" % ("true" if nt else "false", ", true" if exp == e["rowwin"] else "")
        return dict(_walk(total // 4, k), kernel=name, ppt=4, streaming=nt)
    if w >= 2:
        return dict(_walk(total, k), kernel="grid_sample_fwd2_kernel<1, false>", ppt=1, streaming=False)
    if four:
        return dict(_walk(total // 4, k), kernel="grid_sample_fwd_kernel<4>", ppt=4, streaming=False)
    return dict(_walk(total, k), kernel="grid_sample_fwd_kernel<1>", ppt=1, streaming=False)


def dispatch_bwd(n, c, h, w, ho, wo, ginput, aligned=True, exp=0, k=None):
    """pws_grid_sample_bwd: the field-only kernel (4 pixels per lane) or the general one (one pixel per lane, never streaming)"""
    k = k or source_constants()
    total = n * ho * wo
    if not ginput and (ho * wo) % 4 == 0 and w >= 2 and aligned and exp != k["exp"]["general"]:
        nt = _streams(k, "bwd", total, c)
        return dict(_walk(total // 4, k), kernel="grid_sample_bwd_field_kernel<%s>" % ("true" if nt else "false"), ppt=4, streaming=nt)
    return dict(_walk(total, k), kernel="grid_sample_bwd_kernel", ppt=1, streaming=False)


def fused_rx(w, fw):
    """the entry point's fp32 column ratio"""
    return np.float32(fw - 1) / np.float32(w - 1) if w > 1 else np.float32(0)


def dispatch_fused(n, c, h, w, fh, fw, aligned=True, exp=0, k=None):
    """pws_upsample_grid_sample_fwd: <pixels per lane, NARROW, streaming>"""
    k = k or source_constants()
    e = k["exp"]
    total = n * h * w
    if w % 4 == 0 and aligned:
        nt = exp not in (e["general"], e["cvt"], e["rowwin"]) and _streams(k, "fused", total, c)
        span, below = k["narrow"]
        narrow = bool(np.float32(span * fused_rx(w, fw)) < below)
        name = "upsample_grid_sample_fwd_kernel<4, %s, %s>" % ("true" if narrow else "false", "true" if narrow and nt else "false")
        return dict(_walk(total // 4, k), kernel=name, ppt=4, narrow=narrow, streaming=narrow and nt)
    return dict(_walk(total, k), kernel="upsample_grid_sample_fwd_kernel<1, false, false>", ppt=1, narrow=False, streaming=False)
