"""float64 restatement of the training-objective kernels (csrc/objective.hip), the input builders that make every compared element
well-conditioned, and the dispatch arithmetic of the launches -- TEST INFRASTRUCTURE for tests/test_hip_objective_float64.py, held to
torch's float64 grid_sample / affine_grid / autograd and to oracle/objective_ref.py by tests/test_objective_ref64_cpu.py.

One plain function per kernel, torch float64 on whatever device the inputs live on.  Inputs are the fp32 values the kernel sees,
promoted to double; nothing here is rounded to fp32 on the way.

Builders.  The gradient of a bilinear sample with respect to its coordinate is piecewise (it jumps at every cell boundary), and the
gradient of an L1 term flips with the sign of its argument: a test that compares such gradients needs inputs on which no fp32
evaluation can land on the other side.  make_warp_field keeps every sample 0.1 px or more from a cell boundary (fp32 coordinate
rounding is ~W/2 * 2^-24 px), l1_target / make_temporal_case put every L1 argument 0.05 or more from zero, make_shape_resid asserts
that no projection residual is within 1e-9 of zero, make_features keeps every point 0.1 px or more from an index boundary."""
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _d(t):
    return None if t is None else t.to(torch.float64)


# ------------------------------------------------------------------------------------------------------------ bilinear taps
def _unnorm(g, size):
    """align_corners=False: ((g + 1) * size - 1) / 2"""
    return g * (0.5 * size) + 0.5 * (size - 1)


class _Taps:
    """The four taps of bilinear samples at normalised (gx, gy) of an H x W plane, zero padding: flat clamped offsets (o), weights
    with the out-of-frame taps zeroed (w), validity (v) in the order 00, 01, 10, 11 (y, x), and the 1-D weights."""

    def __init__(self, gx, gy, H, W):
        ix, iy = _unnorm(gx, W), _unnorm(gy, H)
        x0, y0 = torch.floor(ix), torch.floor(iy)
        self.wx1, self.wy1 = ix - x0, iy - y0
        self.wx0, self.wy0 = 1.0 - self.wx1, 1.0 - self.wy1
        x0, y0 = x0.long(), y0.long()
        self.x0, self.y0 = x0, y0
        self.o, self.w, self.v = [], [], []
        for dy, wy in ((0, self.wy0), (1, self.wy1)):
            for dx, wx in ((0, self.wx0), (1, self.wx1)):
                xi, yi = x0 + dx, y0 + dy
                valid = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
                self.o.append(yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1))
                self.v.append(valid)
                self.w.append(torch.where(valid, wx * wy, torch.zeros_like(wx)))

    def values(self, img):
        """img (m, C, H, W) -> the four tap values (m, C, ...) with zeros outside the frame"""
        m, C = img.shape[0], img.shape[1]
        flat = img.reshape(m, C, -1)
        out = []
        for o, v in zip(self.o, self.v):
            val = flat.gather(2, o.reshape(m, 1, -1).expand(m, C, -1)).reshape((m, C) + tuple(o.shape[1:]))
            out.append(val * v.unsqueeze(1).to(img.dtype))
        return out


# ------------------------------------------------------------------------------------------------------------ warp + L1
def warp_norm(src, grid, target=None, c_l1=0.0, scale=None, gextra=None, ggrid0=None):
    """warp_norm_fwd / warp_norm_bwd: fake = grid_sample((src + 1) * 127.5, grid, align_corners=False, zeros) / 127.5 - 1;
    l1 = sum |target - fake|; gfake = c_l1 * scale * sign(fake - target) + gextra; ggrid = (d fake / d grid)^T gfake (+ ggrid0 when the
    kernel accumulates).  scale multiplies the L1 coefficient only.  Returns fake, d = target - fake, l1, ggrid."""
    src, grid = _d(src), _d(grid)
    m, _, H, W = src.shape
    t = _Taps(grid[..., 0], grid[..., 1], H, W)
    v00, v01, v10, v11 = t.values((src + 1.0) * 127.5)
    wx0, wx1, wy0, wy1 = (a.unsqueeze(1) for a in (t.wx0, t.wx1, t.wy0, t.wy1))
    fake = (v00 * (wx0 * wy0) + v01 * (wx1 * wy0) + v10 * (wx0 * wy1) + v11 * (wx1 * wy1)) / 127.5 - 1.0
    out = {"fake": fake}
    gf = torch.zeros_like(fake) if gextra is None else _d(gextra).clone()
    if target is not None:
        d = _d(target) - fake
        out["d"], out["l1"] = d, d.abs().sum()
        gf = gf + float(c_l1) * (1.0 if scale is None else float(scale)) * torch.sign(-d)
    gix = (gf * ((v01 - v00) * wy0 + (v11 - v10) * wy1)).sum(1) * (0.5 * W / 127.5)
    giy = (gf * ((v10 - v00) * wx0 + (v11 - v01) * wx1)).sum(1) * (0.5 * H / 127.5)
    gg = torch.stack([gix, giy], -1)
    out["ggrid"] = gg if ggrid0 is None else gg + _d(ggrid0)
    return out


# ------------------------------------------------------------------------------------------------------------ temporal L1
def affine_grid(theta, H, W):
    """F.affine_grid(theta, (n, C, H, W), align_corners=False): base coordinate of pixel j is (2 j + 1) / size - 1"""
    th = _d(theta).reshape(-1, 6)
    bx = ((2.0 * torch.arange(W, dtype=torch.float64, device=th.device) + 1.0) / W - 1.0).reshape(1, 1, W)
    by = ((2.0 * torch.arange(H, dtype=torch.float64, device=th.device) + 1.0) / H - 1.0).reshape(1, H, 1)
    c = [th[:, k].reshape(-1, 1, 1) for k in range(6)]
    return c[0] * bx + c[1] * by + c[2], c[3] * bx + c[4] * by + c[5]


def temporal_l1(fake1, fake2, theta, c=0.0, scale=None, gfake1_0=None, gfake2_0=None):
    """temporal_l1 fwd / bwd / bwd_det: o21 = grid_sample(fake2, affine_grid(theta)); d = o21 - fake1; sum = sum |d|;
    gfake1 = gfake1_0 - c * scale * sign(d); gfake2 = gfake2_0 + the adjoint of the warp applied to c * scale * sign(d)."""
    fake1, fake2 = _d(fake1), _d(fake2)
    n, C, H, W = fake1.shape
    gx, gy = affine_grid(theta, H, W)
    t = _Taps(gx, gy, H, W)
    vals = t.values(fake2)
    o21 = sum(v * w.unsqueeze(1) for v, w in zip(vals, t.w))
    d = o21 - fake1
    out = {"o21": o21, "d": d, "sum": d.abs().sum()}
    s = float(c) * (1.0 if scale is None else float(scale)) * torch.sign(d)
    out["gfake1"] = -s if gfake1_0 is None else _d(gfake1_0) - s
    g2 = (torch.zeros_like(fake2) if gfake2_0 is None else _d(gfake2_0).clone()).reshape(n, C, -1)
    for o, w in zip(t.o, t.w):
        g2.scatter_add_(2, o.reshape(n, 1, -1).expand(n, C, -1), (s * w.unsqueeze(1)).reshape(n, C, -1))
    out["gfake2"] = g2.reshape(n, C, H, W)
    return out


# ------------------------------------------------------------------------------------------------------------ feature points
def feat_index(coord, size):
    """feat_index: int((coord + 1) * size / 2) truncated toward zero; a negative index wraps once (Python indexing); then the clamp"""
    i = torch.trunc((_d(coord) + 1.0) * size / 2.0).long()
    i = torch.where(i < 0, i + size, i)
    return i.clamp(0, size - 1)


def feature_loss(grid, features, c=0.0, scale=None, ggrid0=None):
    """feature_loss fwd / bwd / bwd_det: features (m, nf, 6) = [stable x, y, 1, unstable x, y, 1]; term = |unstable - grid[stable]|^2;
    ggrid[pixel] += -2 c scale (unstable - grid[pixel]) for every point of the pixel (points that share a pixel add up)."""
    grid, f = _d(grid), _d(features)
    m, H, W, _ = grid.shape
    ix, iy = feat_index(f[..., 0], W), feat_index(f[..., 1], H)
    q = ((torch.arange(m, device=grid.device).reshape(m, 1) * H + iy) * W + ix).reshape(-1)
    d = f[..., 3:5].reshape(-1, 2) - grid.reshape(-1, 2)[q]
    terms = (d * d).sum(-1)
    gg = (torch.zeros_like(grid) if ggrid0 is None else _d(ggrid0).clone()).reshape(-1, 2)
    gg.index_add_(0, q, -2.0 * float(c) * (1.0 if scale is None else float(scale)) * d)
    return {"terms": terms.reshape(m, -1), "sum": terms.sum(), "ggrid": gg.reshape(grid.shape), "pixel": q.reshape(m, -1)}


# ------------------------------------------------------------------------------------------------------------ smoothness
def field_smoothness(grid):
    """field_smoothness: sum |grid[:, :, x] - grid[:, :, x + 1]| and sum |grid[:, y] - grid[:, y + 1]| over both coordinates"""
    g = _d(grid)
    tx, ty = (g[:, :, :-1] - g[:, :, 1:]).abs(), (g[:, :-1] - g[:, 1:]).abs()
    return {"dx": tx.sum(), "dy": ty.sum(), "terms_dx": tx, "terms_dy": ty}


# ------------------------------------------------------------------------------------------------------------ shape loss
def shape_basis(block):
    """(block^2, 4) bilinear weights of a block's four corners, pixel-major (y * block + x): oracle/objective_ref.py shape_basis"""
    L = float(block - 1)
    y, x = np.meshgrid(np.arange(block, dtype=np.float64), np.arange(block, dtype=np.float64), indexing="ij")
    x, y = x.reshape(-1), y.reshape(-1)
    return np.stack([(L - x) * (L - y), x * (L - y), (L - x) * y, x * y], axis=1) / (L * L)


def shape_projector(block):
    """The explicit A (A^T A)^-1 A^T"""
    a = shape_basis(block)
    return a @ np.linalg.inv(a.T @ a) @ a.T


def shape_loss(resid, block, c=0.0, scale=None):
    """shape_loss fwd / bwd: every block x block patch B of the (m, size, size, 2) residual field (size == block^2) against its
    projection P B; sum = sum |P B - B|; gresid = c * scale * (P s - s), s = sign(P B - B).  Also returns r = P B - B per patch."""
    r64 = _d(resid)
    m, size = r64.shape[0], r64.shape[1]
    bs = size // block
    assert bs == block and size == block * block
    P = torch.from_numpy(shape_projector(block)).to(r64.device)
    b = r64.reshape(m, block, bs, block, bs, 2).permute(0, 1, 3, 2, 4, 5).reshape(-1, bs * bs, 2)
    r = P @ b - b
    s = torch.sign(r)
    g = float(c) * (1.0 if scale is None else float(scale)) * (P @ s - s)
    g = g.reshape(m, block, block, bs, bs, 2).permute(0, 1, 3, 2, 4, 5).reshape(m, size, size, 2)
    return {"sum": r.abs().sum(), "r": r, "gresid": g}


# ------------------------------------------------------------------------------------------------------------ finalize
def finalize(slots, coef):
    """objective_finalize: out[j] = sum_q coef[j, q] * (sum of quantity q's slots)"""
    return _d(coef) @ _d(slots).sum(1)


# ------------------------------------------------------------------------------------------------------------ input builders
def u8_frames(rs, shape):
    """uniform random 8-bit frames normalised as u8_normalize does (x * (1/255) * 2 - 1 in fp32): the worst image gradients"""
    u8 = rs.randint(0, 256, shape).astype(np.float32)
    return u8 * np.float32(1.0 / 255) * np.float32(2) - np.float32(1)


def smooth_frames(m, c, H, W, seed):
    """synth.make_frames normalised the same way"""
    from pwstablenet_amd import synth
    fr = np.round(synth.make_frames(m, c, H, W, seed=seed)).astype(np.float32)
    return fr * np.float32(1.0 / 255) * np.float32(2) - np.float32(1)


FRAC_LO, FRAC_HI = 0.1, 0.9
INT_LO, INT_PAST = -3, 2          # integer parts of the sample coordinates run over [-3, size + 2]
FAR = 8                           # samples put 5 frame widths outside the frame


def make_warp_field(m, H, W, seed):
    """(m, H, W, 2) fp32 field built from PIXEL coordinates: integer part uniform over [-3, size + 2] in both axes (x0 = -1, x0 = W - 1,
    y0 = -1, y0 = H - 1, taps fully outside, every `sel` branch of the paired loads), fraction uniform over [0.1, 0.9]; the last pixels of
    sample 0 sit on the frame's corners and edges whatever the draw (a 2 x 2 frame has four pixels to draw); the first
    min(FAR, pixels / 4) samples of the last sample lie 5 frame widths outside.  Normalised in double, then rounded to fp32.  Returns the
    field and the pixel coordinates (double) it was built from."""
    rs = np.random.RandomState(seed)
    px = rs.randint(INT_LO, W + INT_PAST + 1, (m, H, W)) + rs.uniform(FRAC_LO, FRAC_HI, (m, H, W))
    py = rs.randint(INT_LO, H + INT_PAST + 1, (m, H, W)) + rs.uniform(FRAC_LO, FRAC_HI, (m, H, W))
    far = min(FAR, H * W // 4)
    corners = [(-1, -1), (W - 1, H - 1), (0, 0), (-1, H - 1), (W - 1, -1), (0, -1)][:H * W - far]     # (x0, y0) of sample 0's last pixels
    cx, cy = px[0].reshape(-1), py[0].reshape(-1)              # views
    for k, (x0, y0) in enumerate(corners):
        i = H * W - 1 - k
        cx[i], cy[i] = x0 + (cx[i] - np.floor(cx[i])), y0 + (cy[i] - np.floor(cy[i]))
    sgn = np.where(np.arange(far) % 2 == 0, -5.0, 6.0)
    fx, fy = px[m - 1].reshape(-1), py[m - 1].reshape(-1)      # views
    fx[:far] = sgn * W + rs.uniform(FRAC_LO, FRAC_HI, far)
    fy[far // 2:far] = sgn[far // 2:] * H + rs.uniform(FRAC_LO, FRAC_HI, far - far // 2)
    g = np.stack([(2.0 * px + 1.0) / W - 1.0, (2.0 * py + 1.0) / H - 1.0], -1).astype(np.float32)
    return torch.from_numpy(g), px, py


def l1_target(value64, rs):
    """fp32(value + s u), s = +-1 at random, u in [0.05, 1]: the sign of (target - value) is the same in any sane fp32 evaluation"""
    shape = tuple(value64.shape)
    su = np.where(rs.randint(0, 2, shape) == 0, -1.0, 1.0) * rs.uniform(0.05, 1.0, shape)
    tgt = (value64.cpu() + torch.from_numpy(su)).to(torch.float32)
    gap = float((tgt.double() - value64.cpu()).abs().min())
    assert gap >= 0.04, gap
    return tgt


def make_warp_case(m, H, W, seed=0, source="u8", device="cpu"):
    """Inputs of one warp + L1 case, fp32 on the CPU: frames (m, 6, H, W) -- channels 0:3 the source, 3:6 the L1 target with decided
    signs --, the field, and the float64 forward (fake, d, l1) on `device`."""
    rs = np.random.RandomState(1000 + seed)
    grid, px, py = make_warp_field(m, H, W, seed)
    src = torch.from_numpy(u8_frames(rs, (m, 3, H, W)) if source == "u8" else smooth_frames(m, 3, H, W, seed + 5))
    fake64 = warp_norm(src.to(device), grid.to(device))["fake"]
    target = l1_target(fake64, rs)
    d64 = target.to(device).double() - fake64
    assert float(d64.abs().min()) >= 0.04
    return {"frames": torch.cat([src, target], 1), "grid": grid, "px": px, "py": py, "fake64": fake64, "d64": d64, "l1_64": d64.abs().sum()}


THETAS = {"near identity": [1, 0, 0, 0, 1, 0], "rotation + zoom": [0.8, 0.5, 0.05, -0.45, 0.7, -0.1],
          "leaves the frame": [1.3, 0.1, 0.6, 0.0, 1.2, -0.7], "degenerate": [1, 0.5, 0, 2, 1, 0]}


def make_theta(kind, n, seed=0):
    """the four kinds of test_temporal_l1_backward_without_atomics_equals_the_scatter: base + 0.02 of noise (none on the singular one)"""
    rs = np.random.RandomState(77 + seed)
    noise = rs.standard_normal((n, 6)).astype(np.float32) * np.float32(0.0 if kind == "degenerate" else 0.02)
    return torch.from_numpy(np.asarray([THETAS[kind]], np.float32).repeat(n, 0) + noise)


def make_temporal_case(n, H, W, kind, seed=0, device="cpu"):
    """fake2 = uniform random 8-bit frames; fake1 = fp32(warp64(fake2, theta) + s u): every sign(d) decided (min |d64| >= 0.04)."""
    rs = np.random.RandomState(2000 + seed)
    fake2 = torch.from_numpy(u8_frames(rs, (n, 3, H, W)))
    theta = make_theta(kind, n, seed)
    zero = torch.zeros((n, 3, H, W), dtype=torch.float64, device=device)
    o21 = temporal_l1(zero, fake2.to(device), theta.to(device))["o21"]
    fake1 = l1_target(o21, rs)
    return {"fake1": fake1, "fake2": fake2, "theta": theta}


SIGN_GAP = 1e-9                   # no shape residual |P B - B| closer to zero than this


def make_shape_resid(m, size, seed=0, block=None, device="cpu"):
    """(m, size, size, 2) fp32: a smooth field plus uniform noise of amplitude 1e-2.  With `block`: sign(P B - B) is decided -- among
    millions of residuals of ~1e-2 a few land within 1e-9 of zero by chance; the noise of those pixels is drawn again until none does
    (the kernel works in double on the same fp32 input, its rounding is ~1e-17)."""
    rs = np.random.RandomState(3000 + seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, size), np.linspace(0, 1, size), indexing="ij")
    smooth = np.empty((m, size, size, 2), np.float64)
    for i in range(m):
        for c in range(2):
            fx, fy, ph = rs.uniform(0.5, 4), rs.uniform(0.5, 4), rs.uniform(0, 6.28)
            smooth[i, :, :, c] = 0.05 * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph)
    resid = torch.from_numpy((smooth + rs.uniform(-1e-2, 1e-2, smooth.shape)).astype(np.float32))
    if block is None:
        return resid
    bs = size // block
    for _ in range(20):
        r = shape_loss(resid.to(device), block)["r"]
        close = (r.abs() <= 100 * SIGN_GAP).reshape(m, block, block, bs, bs, 2).permute(0, 1, 3, 2, 4, 5).reshape(m, size, size, 2).cpu().numpy()
        if not close.any():
            break
        again = (smooth[close] + rs.uniform(-1e-2, 1e-2, int(close.sum()))).astype(np.float32)
        resid[torch.from_numpy(close)] = torch.from_numpy(again)
    check_shape_resid(resid, block, device)
    return resid


def check_shape_resid(resid, block, device="cpu"):
    """asserts min |P B - B| > 1e-9 on the float64 reference; returns it"""
    r = shape_loss(resid.to(device), block)["r"]
    gap = float(r.abs().min())
    assert gap > SIGN_GAP, gap
    return gap


def make_features(m, nf, H, W, seed=0, edges=True):
    """(m, nf, 6) fp32: stable points at pixel index + [0.1, 0.9] inside [-0.96, 0.96] (no index within 0.1 px of a boundary), the
    second quarter of a sample's points on the pixels of the first quarter, unstable = stable + N(0, 0.03); with `edges` (nf >= 8) the
    last four points of sample 0 get x = -1.0, 0.999, -1.004, -1.02 (index 0, size - 1, 0, size - 2 by the wrap)."""
    rs = np.random.RandomState(4000 + seed)

    def coords(size):
        lo, hi = int(np.ceil(0.02 * size)), int(np.floor(0.98 * size)) - 1        # indices whose whole pixel lies in [-0.96, 0.96]
        lo, hi = (0, size - 1) if hi < lo else (lo, hi)
        idx = rs.randint(lo, hi + 1, (m, nf))
        return idx, (idx + rs.uniform(FRAC_LO, FRAC_HI, (m, nf))) * 2.0 / size - 1.0
    ix, sx = coords(W)
    iy, sy = coords(H)
    q = nf // 4
    if q:
        sx[:, q:2 * q], sy[:, q:2 * q] = sx[:, :q], sy[:, :q]
        ix[:, q:2 * q], iy[:, q:2 * q] = ix[:, :q], iy[:, :q]
    if edges and nf >= 8:
        sx[0, nf - 4:] = [-1.0, 0.999, -1.004, -1.02]
    one = np.ones((m, nf, 1))
    st = np.stack([sx, sy], -1)
    un = st + rs.normal(0, 0.03, st.shape)
    return torch.from_numpy(np.concatenate([st, one, un, one], 2).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ dispatch arithmetic
def source_constants():
    """kLossGrid, kXcds, the slot count and the lanes per workgroup, read from the sources' text"""
    def grab(path, pattern):
        with open(os.path.join(ROOT, path)) as f:
            mt = re.search(pattern, f.read())
        assert mt, (path, pattern)
        return int(mt.group(1))
    return {"kLossGrid": grab("pwstablenet_amd/csrc/objective.hip", r"constexpr\s+unsigned\s+kLossGrid\s*=\s*(\d+)\s*;"),
            "kXcds": grab("pwstablenet_amd/csrc/common.h", r"constexpr\s+int\s+kXcds\s*=\s*(\d+)\s*;"),
            "slots": grab("include/pwstable.h", r"#define\s+PWS_OBJ_SLOTS\s+(\d+)"),
            "lanes": grab("pwstablenet_amd/csrc/objective.hip", r"__launch_bounds__\((\d+)\)\s+warp_norm_fwd_kernel")}


def _walk(units, capped_launch, k):
    """`units` lanes' worth of work in blocks of 256 lanes on a grid that a capped launch limits to kLossGrid workgroups"""
    nb = -(-units // k["lanes"])
    capped = capped_launch and nb > k["kLossGrid"]
    return {"nb": nb, "capped": capped, "grid": k["kLossGrid"] if capped else nb, "mod8": nb % k["kXcds"], "ragged": units % k["lanes"] != 0}


def dispatch_warp_fwd(m, h, w, k=None):
    k = k or source_constants()
    if (h * w) % 4 != 0 or w < 2:
        return {"kernel": "refused"}
    return dict(_walk(m * h * w // 4, True, k), kernel="warp_norm_fwd_kernel")


def dispatch_warp_bwd(m, h, w, k=None):
    k = k or source_constants()
    if (h * w) % 4 == 0 and w >= 2:
        return dict(_walk(m * h * w // 4, False, k), kernel="warp_norm_bwd4_kernel")
    return dict(_walk(m * h * w, False, k), kernel="warp_norm_bwd_kernel")


def dispatch_temporal(n, h, w, k=None):
    """forward walk (capped) and the backward's g_pair"""
    k = k or source_constants()
    total = n * h * w
    return dict(_walk(total, True, k), kernel="temporal_l1_kernel", g_pair=0 if (total % k["lanes"] != 0 or (h * w) % 64 != 0) else 1,
                wave_spans_rows=w < 64 or w % 64 != 0)


def dispatch_smooth(m, h, w, one_pixel=False, k=None):
    k = k or source_constants()
    if w % 4 == 0 and not one_pixel:
        return dict(_walk(m * h * w // 4, True, k), kernel="field_smoothness4_kernel")
    return dict(_walk(m * h * w, True, k), kernel="field_smoothness_kernel")


def dispatch_shape(m, size, block, general=False, k=None):
    """wave kernel: one WAVE per block, 4 waves per workgroup, the grid capped; general kernel: one workgroup per block"""
    k = k or source_constants()
    assert size == block * block
    nb, bs = m * block * block, size // block
    if bs == 16 and not general:
        grid = -(-nb // 4)
        capped = grid > k["kLossGrid"]
        grid = k["kLossGrid"] if capped else grid
        return {"kernel": "shape_loss16_kernel", "nb": nb, "capped": capped, "grid": grid, "waves": grid * 4}
    return {"kernel": "shape_loss_kernel", "nb": nb, "capped": False, "grid": nb, "threads": -(-bs * bs // 64) * 64, "live": bs * bs}


def dispatch_feature(m, nf, k=None):
    k = k or source_constants()
    return dict(_walk(m * nf, False, k), kernel="feature_loss_kernel")
