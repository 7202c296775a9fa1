"""The two regression heads, forward and backward, against float64 torch autograd on the CPU -- at the batch sizes that pick the
kernels' multi-slice paths (theta_bwd1_kernel deals samples to up to 8 workgroups per hidden block from n = 16 on; field_gz_kernel's
pixel slices depend on n and h*w) -- plus the bf16 <-> fp32 copies the theta head goes through under bf16 storage, and the whole
generator's deterministic mode at training batches.

Tolerances are relative to the tensor's largest float64 value.  fp32 paths: the length of the longest chain of fp32 roundings that
forms one element, times ULP32 = 8 * 2^-24: 2^-24 per rounding bounds the error relative to the sum of the terms' magnitudes, and the
factor 8 covers the ratio of that sum to the tensor's largest value (random-sign terms); chains are counted per call below.  bf16
paths: 2^-8 (half a bf16 ulp) per rounding -- of a stored result, or of each operand that enters a matrix-core product (2^-7 per
product).  Each bound carries the largest error measured on an MI355X over the test's cases in brackets.
"""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402
from pwstablenet_amd.hipabi import Exp  # noqa: E402

pytestmark = pytest.mark.gpu

from pwstablenet_amd import synth  # noqa: E402

ULP32 = 8 * 2.0 ** -24


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel_err(got, want):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def check_rel(name, got, want, tol):
    err = rel_err(got, want)
    assert err <= tol, "%s: max err / max|f64| = %.3g (bound %.3g)" % (name, err, tol)
    return err


def lrelu_fixed(z, mask):
    """LeakyReLU 0.2 with its branch given: autograd differentiates exactly the branch taken."""
    return torch.where(mask, z, 0.2 * z)


# ------------------------------------------------------------------------------------------------------------ theta head
def _theta_slices(n):
    return 1 if n < 16 else min(n // 8, 8)   # head_bwd.hip theta_bwd1_slices (not deterministic)


THETA_N = [1, 2, 15, 16, 17, 23, 63, 64, 65, 100, 517]
THETA_SHAPES = [(512, 512), (64, 300), (512, 64)]   # (c, hidden): the product, a partial last hidden block, a small hidden layer


@pytest.mark.parametrize("c,hidden", THETA_SHAPES)
@pytest.mark.parametrize("n", THETA_N)
def test_theta_head_fwd_bwd_vs_float64(hip, n, c, hidden):
    """pws_theta_head_fwd_save + pws_theta_head_bwd against float64 autograd of theta = L(W2 L(W1 vec(x) + b1) + b2).
    Every batch size, including those where the samples do not divide evenly over the slices; weight gradients are accumulated
    onto nonzero contents, dx is overwritten (dx_accumulate 0) and accumulated (1)."""
    A = hip
    L, st = A.lib(), A.current_stream()
    rs = np.random.RandomState(zlib.crc32(repr(("theta", n, c, hidden)).encode()))
    x = rs.standard_normal((n, 2, 2, c))                                   # NHWC
    wf = rs.standard_normal((hidden, c, 2, 2)) / np.sqrt(4 * c)
    bf = rs.standard_normal(hidden) * 0.5                                  # pre-activations of both signs
    wl = rs.standard_normal((6, hidden, 1, 1)) / np.sqrt(hidden)
    bl = rs.standard_normal(6) * 0.5
    dtheta = rs.standard_normal((n, 6))
    f32 = lambda a: np.asarray(a, np.float32)   # noqa: E731

    kl = (hidden + 15) // 16 * 16   # K1 packing pads the input channels (rows of [hidden][6]) to a multiple of 16
    pf = torch.empty(L.pws_packed_weight_floats(A.CONV_K2S1P0, c, hidden), device="cuda")
    pl = torch.empty(L.pws_packed_weight_floats(A.CONV_K1, hidden, 6), device="cuda")
    assert pl.numel() == kl * 6
    d_wf, d_wl = dev(f32(wf)), dev(f32(wl))
    A.check(L.pws_pack_conv_weight(A.ptr(d_wf), A.ptr(pf), A.CONV_K2S1P0, c, hidden, st), "pack flatten")
    A.check(L.pws_pack_conv_weight(A.ptr(d_wl), A.ptr(pl), A.CONV_K1, hidden, 6, st), "pack linear")
    d_x, d_bf, d_bl = dev(f32(x)), dev(f32(bf)), dev(f32(bl))
    theta = torch.full((n, 6), float("nan"), device="cuda")
    hs = torch.full((n, hidden), float("nan"), device="cuda")
    tws = torch.empty(L.pws_theta_head_ws_floats(n, c, hidden), device="cuda")
    A.check(L.pws_theta_head_fwd_save(A.ptr(d_x), n, c, hidden, A.ptr(pf), A.ptr(d_bf), A.ptr(pl), A.ptr(d_bl), A.ptr(tws), A.ptr(theta),
                                      A.ptr(hs), st), "theta fwd")

    # ---- float64 reference; the LeakyReLU branches are those of the kernel's forward, which must agree with float64 wherever the
    # pre-activation is farther than rounding from 0 (at +-1e-6 of the pre-activations' scale the derivative is not defined by fp32)
    torch.cuda.synchronize()
    h_k, th_k = hs.cpu().double(), theta.cpu().double()
    X = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    Wf, Bf = torch.from_numpy(wf).requires_grad_(True), torch.from_numpy(bf).requires_grad_(True)
    Wl, Bl = torch.from_numpy(wl).requires_grad_(True), torch.from_numpy(bl).requires_grad_(True)
    z1 = F.conv2d(X, Wf, Bf).view(n, hidden)
    m1 = h_k > 0
    far1 = z1.detach().abs() > 1e-5 * float(z1.detach().abs().max())
    assert bool(((z1.detach() > 0) == m1)[far1].all()), "hidden LeakyReLU branch differs from float64"
    h = lrelu_fixed(z1, m1)
    z2 = F.conv2d(h.view(n, hidden, 1, 1), Wl, Bl).view(n, 6)
    m2 = th_k > 0
    far2 = z2.detach().abs() > 1e-5 * float(z2.detach().abs().max())
    assert bool(((z2.detach() > 0) == m2)[far2].all()), "theta LeakyReLU branch differs from float64"
    th = lrelu_fixed(z2, m2)
    (th * torch.from_numpy(dtheta)).sum().backward()
    assert 0 < int(m1.sum()) < m1.numel() and 0 < int(m2.sum()) < m2.numel() or n * 6 < 8, "both LeakyReLU branches exercised"
    # forward: z1 sums 4c products and a bias (chain 4c + 1), theta 6 more steps over `hidden` terms
    errs = {"h_saved": check_rel("h_saved", hs, h.detach(), (4 * c + 2) * ULP32),                    # [3.4e-7]
            "theta": check_rel("theta", theta, th.detach(), (4 * c + hidden + 4) * ULP32)}          # [3.3e-7]

    # ---- backward: weight gradients accumulate onto nonzero contents
    pre = lambda shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).cuda()   # noqa: E731
    dwf, dbf, dwl, dbl = pre(pf.numel()), pre(hidden), pre(pl.numel()), pre(6)
    dwf0, dbf0, dwl0, dbl0 = dwf.clone(), dbf.clone(), dwl.clone(), dbl.clone()
    dx_old = pre((n, 2, 2, c))
    d_dth = dev(f32(dtheta))
    ws = torch.full((n * hidden,), float("nan"), device="cuda")
    results = {}
    for acc in (0, 1):
        dx = dx_old.clone()
        A.check(L.pws_theta_head_bwd(A.ptr(d_x), n, c, hidden, A.ptr(pf), A.ptr(pl), A.ptr(hs), A.ptr(theta), A.ptr(d_dth), A.ptr(dwf),
                                     A.ptr(dbf), A.ptr(dwl), A.ptr(dbl), A.ptr(dx), acc, A.ptr(ws), st), "theta bwd")
        torch.cuda.synchronize()
        results[acc] = dx.cpu().double()

    def unpack(p, kind, cin, cout, shape):
        out = torch.empty(shape, device="cuda")
        A.check(L.pws_unpack_conv_weight(A.ptr(p), A.ptr(out), kind, cin, cout, st), "unpack")
        return out.cpu().double()
    # two calls: every weight gradient holds its prefill + 2 x the gradient
    g_wf = (unpack(dwf, A.CONV_K2S1P0, c, hidden, (hidden, c, 2, 2)) - unpack(dwf0, A.CONV_K2S1P0, c, hidden, (hidden, c, 2, 2))) / 2
    g_wl = (unpack(dwl, A.CONV_K1, hidden, 6, (6, hidden, 1, 1)) - unpack(dwl0, A.CONV_K1, hidden, 6, (6, hidden, 1, 1))) / 2
    g_bf, g_bl = (dbf.cpu().double() - dbf0.cpu().double()) / 2, (dbl.cpu().double() - dbl0.cpu().double()) / 2
    assert torch.equal(dwl[hidden * 6:], dwl0[hidden * 6:]), "rows of the K1 packing's channel padding were written"
    # chains (fp32 roundings per element):  dz2 = dtheta * L'  (exact);  dW2 / db2 / db1: the slice's samples in order, then one atomic per
    # slice (<= n + 8);  dz1 = W2^T dz2 (6);  dW1: n samples;  dx: `hidden` terms.  Inputs of a chain carry the forward's error (h: 4c + 2).
    # The prefill (O(1)) and the second call add their own roundings at the prefill's scale: 4 more, scaled by max|prefill| / max|grad|
    nsl = _theta_slices(n)
    fwd = 4 * c + 2

    def bound(chain, ref, prefill):
        return (chain + fwd + 4 * float(prefill.abs().max()) / max(float(ref.abs().max()), 1e-30)) * ULP32
    errs["dW_flat"] = check_rel("dW_flat", g_wf, Wf.grad, bound(n + 6, Wf.grad, dwf0))                # [8.5e-7]
    errs["db_flat"] = check_rel("db_flat", g_bf, Bf.grad, bound(n + nsl + 6, Bf.grad, dbf0))          # [5.8e-7]
    errs["dW_lin"] = check_rel("dW_lin", g_wl, Wl.grad, bound(n + nsl, Wl.grad, dwl0))                # [4.0e-7]
    errs["db_lin"] = check_rel("db_lin", g_bl, Bl.grad, bound(n + nsl, Bl.grad, dbl0))                # [2.6e-7]
    gx = X.grad.permute(0, 2, 3, 1)
    errs["dx"] = check_rel("dx (overwritten)", results[0], gx, bound(hidden + 6, gx, torch.zeros(1)))                    # [2.0e-7]
    errs["dx_acc"] = check_rel("dx (accumulated)", results[1] - dx_old.cpu().double(), gx, bound(hidden + 6, gx, dx_old.cpu()))   # [1.9e-6]
    print("theta head n=%d c=%d hidden=%d slices=%d: %s" % (n, c, hidden, nsl, ", ".join("%s %.2g" % kv for kv in errs.items())))


def test_theta_head_edges(hip):
    """n = 0 leaves every output untouched; a batch whose per-slice staging exceeds the 64 KB of LDS is refused with PWS_EINVAL
    before anything is launched (all buffers are still allocated at full size)."""
    A = hip
    L, st = A.lib(), A.current_stream()
    c, hidden = 64, 64
    pf = torch.randn(L.pws_packed_weight_floats(A.CONV_K2S1P0, c, hidden), device="cuda")
    pl = torch.randn(L.pws_packed_weight_floats(A.CONV_K1, hidden, 6), device="cuda")
    outs = [torch.randn(k, device="cuda") for k in (pf.numel(), hidden, pl.numel(), 6)]
    keep = [o.clone() for o in outs]
    for n in (0, 8 * 2731):   # 8 slices of ceil(n / 8) = 2731 samples: 2731 * 24 B = 65544 B > 64 KB
        m = max(n, 1)
        x, hs, th, dth = (torch.randn(m * 4 * c, device="cuda"), torch.randn(m * hidden, device="cuda"), torch.randn(m * 6, device="cuda"),
                          torch.randn(m * 6, device="cuda"))
        dx, ws = torch.randn(m * 4 * c, device="cuda"), torch.empty(m * hidden, device="cuda")
        dx0 = dx.clone()
        rc = L.pws_theta_head_bwd(A.ptr(x), n, c, hidden, A.ptr(pf), A.ptr(pl), A.ptr(hs), A.ptr(th), A.ptr(dth), *[A.ptr(o) for o in outs],
                                  A.ptr(dx), 0, A.ptr(ws), st)
        torch.cuda.synchronize()
        if n == 0:
            assert rc == 0
        else:
            assert rc == -22 and b"LDS" in L.pws_last_error(), (rc, L.pws_last_error())
        assert torch.equal(dx, dx0) and all(torch.equal(a, b) for a, b in zip(outs, keep))
    # one sample below the bound runs
    n = 8 * 2730
    x, hs, th, dth = (torch.randn(n * 4 * c, device="cuda"), torch.randn(n * hidden, device="cuda"), torch.randn(n * 6, device="cuda"),
                      torch.randn(n * 6, device="cuda"))
    ws = torch.empty(n * hidden, device="cuda")
    A.check(L.pws_theta_head_bwd(A.ptr(x), n, c, hidden, A.ptr(pf), A.ptr(pl), A.ptr(hs), A.ptr(th), A.ptr(dth), *[A.ptr(o) for o in outs],
                                 None, 0, A.ptr(ws), st), "theta bwd at the LDS bound")


# ------------------------------------------------------------------------------------------------------------ field head
def _field_ref(x_nhwc, w_out, b_out, theta, ac, g_grid, g_resid):
    """float64: grid = tanh(tanh(conv3x3(x) + b)) + affine_grid(theta); gradients of <grid, g_grid> + <resid, g_resid>."""
    n, h, w, c = x_nhwc.shape
    X = x_nhwc.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    Wt = w_out.double().clone().requires_grad_(True)
    B = b_out.double().clone().requires_grad_(True)
    T = theta.double().clone().requires_grad_(True)
    r = torch.tanh(torch.tanh(F.conv2d(X, Wt, B, padding=1))).permute(0, 2, 3, 1)
    grid = r + F.affine_grid(T.view(n, 2, 3), (n, 2, h, w), align_corners=bool(ac))
    loss = 0
    if g_grid is not None:
        loss = loss + (grid * g_grid.double()).sum()
    if g_resid is not None:
        loss = loss + (r * g_resid.double()).sum()
    loss.backward()
    return r.detach(), grid.detach(), X.grad.permute(0, 2, 3, 1), Wt.grad, B.grad, T.grad


def _field_chains(n, h, w, c):
    """Longest fp32 addition chains of pws_field_head_bwd's kernels (head_bwd.hip, non-deterministic launch shapes)."""
    hw = h * w
    slices = max(1, min((2048 + n - 1) // n, (hw + 1023) // 1024))
    per_lane = -(-(-(-hw // slices)) // 256)
    gz = per_lane + 8 + n * slices          # lane chain, wave + workgroup tree, atomics of all workgroups (db_out: n * slices of them)
    tiles = -(-w // 16) * -(-h // 16) * n
    gx = min(-(-1024 // -(-c // 32)), tiles)
    dw = 32 * -(-tiles // gx) + 8 + gx     # lane chain over its tiles, 8 groups, one atomic per workgroup
    return dict(dx=18 + 4, dw=dw + 4, db=gz, dtheta=per_lane + 8 + slices)


FIELD_CASES = [   # n, h, w, c, align_corners, inputs ("grid" / "resid" / "both"), dtheta given, dx given
    (1, 256, 256, 64, 0, "both", True, True),
    (2, 256, 256, 32, 1, "grid", True, True),
    (9, 256, 256, 32, 0, "resid", False, True),
    (33, 256, 256, 32, 1, "both", True, True),     # 63 pixel slices per image: max_slices (64) does not bind
    (1, 23, 41, 96, 1, "grid", True, True),
    (2, 23, 41, 64, 0, "both", True, False),
    (9, 23, 41, 96, 1, "resid", True, True),
    (33, 23, 41, 64, 0, "grid", True, True),
]


def _field_inputs(rs, n, h, w, c, which):
    x = torch.from_numpy(rs.standard_normal((n, h, w, c)).astype(np.float32))
    w_out = torch.from_numpy((rs.standard_normal((2, c, 3, 3)) * 0.5 / np.sqrt(9 * c)).astype(np.float32))
    b_out = torch.from_numpy((rs.standard_normal(2) * 0.2).astype(np.float32))
    theta = torch.from_numpy((np.array([1, 0, 0, 0, 1, 0]) + rs.standard_normal((n, 6)) * 0.1).astype(np.float32))
    gg = torch.from_numpy(rs.standard_normal((n, h, w, 2)).astype(np.float32)) if which in ("grid", "both") else None
    gr = torch.from_numpy(rs.standard_normal((n, h, w, 2)).astype(np.float32)) if which in ("resid", "both") else None
    return x, w_out, b_out, theta, gg, gr


def _strided(t, ld, fill, dtype=torch.float32):
    """[n,h,w,c] on the device with pixel stride ld; the padding channels hold `fill`."""
    n, h, w, c = t.shape
    out = torch.full((n, h, w, ld), fill, dtype=dtype, device="cuda")
    out[..., :c] = t.to(dtype).cuda()
    return out


def _run_field(A, x_dev, ld, c, w_out, b_out, theta, ac, gg, gr, store, dx_ld, dx_init, acc, dtheta_on, dx_act=None, fwd=True):
    """forward (resid) then backward; returns resid, grid, dx (device), dW (torch layout) - prefill, db - prefill, dtheta."""
    L, st = A.lib(), A.current_stream()
    n, h, w = x_dev.shape[:3]
    po = torch.empty(L.pws_packed_weight_floats(A.CONV_K3S1_OUT, c, 2), device="cuda")
    d_w = w_out.cuda()
    A.check(L.pws_pack_conv_weight(A.ptr(d_w), A.ptr(po), A.CONV_K3S1_OUT, c, 2, st), "pack out")
    d_b, d_th = b_out.cuda(), theta.cuda()
    resid, grid = torch.full((n, h, w, 2), float("nan"), device="cuda"), torch.full((n, h, w, 2), float("nan"), device="cuda")
    A.check(L.pws_field_head_fwd_s(A.ptr(x_dev), ld, n, h, w, c, A.ptr(po), A.ptr(d_b), A.ptr(d_th), ac, A.ptr(resid), A.ptr(grid), store, st),
            "field fwd")
    dwp = torch.randn(po.numel(), device="cuda")
    dwp0 = dwp.clone()
    db = torch.randn(2, device="cuda")
    db0 = db.clone()
    dth = torch.full((n, 6), 123.0, device="cuda") if dtheta_on else None
    dx = dx_init.clone() if dx_init is not None else None
    ws = torch.full((n * h * w * 2,), float("nan"), device="cuda")
    d_gg = gg.cuda() if gg is not None else None   # held until the call has run
    d_gr = gr.cuda() if gr is not None else None
    args = (A.ptr(x_dev), ld, n, h, w, c, A.ptr(po), A.ptr(resid), A.ptr(d_gg), A.ptr(d_gr), ac, A.ptr(dx), dx_ld, acc, A.ptr(dwp), A.ptr(db), A.ptr(dth), A.ptr(ws), store)
    if dx_act is None:
        A.check(L.pws_field_head_bwd_s(*args, st), "field bwd")
    else:
        A.check(L.pws_field_head_bwd_act(*args, dx_act, st), "field bwd act")
    torch.cuda.synchronize()

    def unpack(p):
        out = torch.empty((2, c, 3, 3), device="cuda")
        A.check(L.pws_unpack_conv_weight(A.ptr(p), A.ptr(out), A.CONV_K3S1_OUT, c, 2, st), "unpack")
        return out.cpu().double()
    return (resid.cpu(), grid.cpu(), dx, unpack(dwp) - unpack(dwp0), (db - db0).cpu().double(), dth.cpu() if dth is not None else None,
            float(dwp0.abs().max()))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n,h,w,c,ac,which,dtheta_on,dx_on", FIELD_CASES)
def test_field_head_fp32_vs_float64(hip, n, h, w, c, ac, which, dtheta_on, dx_on, acc):
    """pws_field_head_fwd_s + pws_field_head_bwd_s (fp32 storage) against float64 autograd: dx (pixel stride dx_ld > c, overwritten or
    accumulated), dW_out and db_out (accumulated onto nonzero contents), dtheta (prefilled: overwritten)."""
    A = hip
    rs = np.random.RandomState(zlib.crc32(repr(("field", n, h, w, c, ac, which, acc)).encode()))
    x, w_out, b_out, theta, gg, gr = _field_inputs(rs, n, h, w, c, which)
    r64, grid64, gx64, gw64, gb64, gt64 = _field_ref(x, w_out, b_out, theta, ac, gg, gr)
    ld, dx_ld = c + 8, c + 12
    x_dev = _strided(x, ld, float("nan"))     # the padding channels are never read
    dx_old = torch.randn((n, h, w, c)) * float(gx64.abs().max())
    dx_init = _strided(dx_old, dx_ld, -7.0) if dx_on else None
    resid, grid, dx, gw, gb, gt, pre_w = _run_field(A, x_dev, ld, c, w_out, b_out, theta, ac, gg, gr, A.STORE_FP32, dx_ld, dx_init, acc, dtheta_on)
    ch = _field_chains(n, h, w, c)
    # forward: conv 9c + 1 terms, two tanh (a few ulp each), the affine part 3 terms
    errs = {"resid": check_rel("resid", resid, r64, (9 * c + 16) * ULP32),                                      # [1.8e-6]
            "grid": check_rel("grid", grid, grid64, (9 * c + 20) * ULP32)}                                     # [6.8e-7]
    # the backward reads the forward's fp32 resid: g_z = g (1 - r^2)(1 - atanh(r)^2) carries a few ulp more (chain + 8)
    errs["dW_out"] = check_rel("dW_out", gw, gw64, (ch["dw"] + 8 + 2 * pre_w / float(gw64.abs().max())) * ULP32)  # [9.2e-7]
    errs["db_out"] = check_rel("db_out", gb, gb64, (ch["db"] + 8 + 2 * 4.0 / float(gb64.abs().max())) * ULP32)   # [1.9e-6]
    if dtheta_on:
        if gg is None:
            assert float(gt.abs().max()) == 0.0
        else:
            errs["dtheta"] = check_rel("dtheta", gt, gt64, (ch["dtheta"] + 4) * ULP32)                        # [3.1e-7]
    if dx_on:
        got = dx.cpu()
        assert bool((got[..., c:] == -7.0).all()), "dx padding channels written"
        d = got[..., :c].double() - (dx_old.double() if acc else 0)
        errs["dx"] = check_rel("dx", d, gx64, (ch["dx"] + 8 + (4 * float(dx_old.abs().max()) / float(gx64.abs().max()) if acc else 0)) * ULP32)  # [5.8e-7]
    print("field head fp32 n=%d %dx%d c=%d ac=%d %s: %s" % (n, h, w, c, ac, which, ", ".join("%s %.2g" % kv for kv in errs.items())))


BF16_CASES = [   # n, h, w, c, align_corners, inputs
    (2, 23, 41, 64, 1, "both"),
    (9, 23, 41, 32, 0, "grid"),
    (1, 256, 256, 64, 0, "resid"),
    (33, 23, 41, 96, 1, "both"),
]


@pytest.mark.parametrize("act", ["ACT_NONE", "ACT_RELU", "ACT_LRELU"])
@pytest.mark.parametrize("valu", [False, True])
@pytest.mark.parametrize("n,h,w,c,ac,which", BF16_CASES)
def test_field_head_bf16_vs_float64(hip, n, h, w, c, ac, which, valu, act):
    """bf16 storage against float64 of the same bf16-rounded x: the c == 64 matrix-core kernel (field_bwd16_mfma_kernel: g_z and W_out
    enter the products as bf16) and the VALU kernels (PWS_OPT_EXPERIMENT 91; every other c takes them anyway: fp32 products), each with
    pws_field_head_bwd_act -- dx (accumulated) times act'(x), with some x exactly +-0 (act'(0) is the negative branch)."""
    A = hip
    rs = np.random.RandomState(zlib.crc32(repr(("field16", n, h, w, c, ac, which, valu, act)).encode()))
    x, w_out, b_out, theta, gg, gr = _field_inputs(rs, n, h, w, c, which)
    x = x.bfloat16().float()
    flat = x.view(-1)
    zeros = torch.from_numpy(rs.choice(flat.numel(), flat.numel() // 50, replace=False))
    flat[zeros] = 0.0
    flat[zeros[::2]] = -0.0
    r64, grid64, gx64, gw64, gb64, gt64 = _field_ref(x, w_out, b_out, theta, ac, gg, gr)
    slope = {"ACT_NONE": 1.0, "ACT_RELU": 0.0, "ACT_LRELU": 0.2}[act]
    mask = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope)).double() if act != "ACT_NONE" else torch.ones_like(x).double()
    ld = dx_ld = c + 8
    x_dev = _strided(x, ld, 0.0, torch.bfloat16)
    dx_old = (torch.randn((n, h, w, c)) * 0.5 * float(gx64.abs().max())).bfloat16().float()
    dx_init = _strided(dx_old, dx_ld, -7.0, torch.bfloat16)
    want_dx = (gx64 + dx_old.double()) * mask
    with A.experiment(Exp.HEAD_BWD_VALU if valu else 0):
        out = _run_field(A, x_dev, ld, c, w_out, b_out, theta, ac, gg, gr, A.STORE_BF16, dx_ld, dx_init, 1, True,
                         dx_act=None if act == "ACT_NONE" else getattr(A, act))
    resid, grid, dx, gw, gb, gt, pre_w = out
    got = dx.cpu().float()
    assert bool((got[..., c:] == -7.0).all()), "dx padding channels written"
    got = got[..., :c].double()
    mfma = c == 64 and not valu
    # dx: one bf16 rounding of the result (2^-8 of the element <= max) after fp32 sums (VALU: 2^-8 + 2^-16 [3.5e-3]); on the matrix
    # cores g_z and W_out also enter the products as bf16: 2^-7 per product, and the 18 products of a sum are of random sign, their
    # absolute sum up to ~2x the largest result -> 2^-6 [3.5e-3]
    tol_dx = 2.0 ** -6 if mfma else 2.0 ** -8 + 2.0 ** -16
    errs = {"dx": check_rel("dx", got, want_dx, tol_dx)}
    # dW_out: x is exact (the reference sees the same bf16 values); matrix cores: g_z rounded to bf16 (2^-8 per product), random-sign
    # sums whose absolute sum is up to ~2x the result -> 2^-7 [2.1e-3]; VALU: fp32 products, the fp32 chain of the fp32 test [7.3e-7]
    ch = _field_chains(n, h, w, c)
    tol_dw = 2.0 ** -7 if mfma else (ch["dw"] + 8 + 2 * pre_w / float(gw64.abs().max())) * ULP32
    errs["dW_out"] = check_rel("dW_out", gw, gw64, tol_dw)
    errs["db_out"] = check_rel("db_out", gb, gb64, (ch["db"] + 8 + 2 * 4.0 / float(gb64.abs().max())) * ULP32)  # [2.7e-6]
    if gg is not None:
        errs["dtheta"] = check_rel("dtheta", gt, gt64, (ch["dtheta"] + 4) * ULP32)                          # [1.4e-7]
    print("field head bf16 %s n=%d %dx%d c=%d %s: %s" % ("mfma" if mfma else "valu", n, h, w, c, act, ", ".join("%s %.2g" % kv for kv in errs.items())))


def test_field_head_edges(hip):
    """n = 0: nothing is launched or written."""
    A = hip
    L, st = A.lib(), A.current_stream()
    c = 32
    bufs = [torch.randn(k, device="cuda") for k in (64, 9 * c * 2, 64, 64, 64, 64, 9 * c * 2, 2, 6, 64)]
    keep = [b.clone() for b in bufs]
    x, w, r, gg, gr, dx, dw, db, dth, ws = bufs
    assert L.pws_field_head_bwd_s(A.ptr(x), c, 0, 4, 4, c, A.ptr(w), A.ptr(r), A.ptr(gg), A.ptr(gr), 0, A.ptr(dx), c, 0, A.ptr(dw), A.ptr(db),
                                  A.ptr(dth), A.ptr(ws), A.STORE_FP32, st) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, keep))


# ------------------------------------------------------------------------------------------------------------ bf16 <-> fp32 copies
def _bits16(t):
    return t.contiguous().view(torch.int16).int() & 0xffff


SPECIAL = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0x3F808001, 0x3F7F8000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000,
                    0xFFC00001, 0x7F800001, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x80008000, 0x00000000,
                    0x80000000, 0x00800000], dtype=np.uint32)   # ties to even (both ways), max finite, +-Inf, NaNs, subnormals, +-0


def _special_f32(count, rs):
    v = rs.standard_normal(count).astype(np.float32)
    k = min(count, SPECIAL.size)
    v[:k] = SPECIAL[:k].view(np.float32)
    if count > 2 * SPECIAL.size:
        v[-SPECIAL.size:] = SPECIAL.view(np.float32)   # in the tail too
    return torch.from_numpy(v)


@pytest.mark.parametrize("count", [0, 1, 7, (1 << 20) + 1])
def test_cvt_bf16_to_f32(hip, count):
    A = hip
    L, st = A.lib(), A.current_stream()
    rs = np.random.RandomState(count)
    src = _special_f32(max(count, 1), rs).bfloat16()[:count]
    d_src = src.cuda()
    dst = torch.full((count + 64,), -3.0, device="cuda")
    A.check(L.pws_cvt_bf16_to_f32(A.ptr(d_src) if count else None, A.ptr(dst), count, st), "cvt bf16 -> f32")
    torch.cuda.synchronize()
    got = dst.cpu()
    assert bool((got[count:] == -3.0).all()), "written past count"
    want = src.float()
    assert torch.equal(got[:count].view(torch.int32), want.view(torch.int32))   # exact, NaN payloads included (a shift)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("count", [0, 2, (1 << 20) + 6])
def test_cvt_f32_to_bf16(hip, count, acc):
    """Round to nearest even (ties both ways), +-Inf, NaN stays NaN, subnormals; accumulate: dst = bf16(float(dst) + src) in fp32."""
    A = hip
    L, st = A.lib(), A.current_stream()
    rs = np.random.RandomState(count + acc)
    src = _special_f32(max(count, 2), rs)[:count]
    old = (torch.from_numpy(rs.standard_normal(count + 64).astype(np.float32))).bfloat16()
    if count:
        old[: min(count, 8)] = torch.tensor([1.0, -1.0, 2.0 ** -133, 0.0, 1.0, 3.0, -2.0 ** -130, 1e30])[: min(count, 8)].bfloat16()
    dst = old.cuda()
    d_src = src.cuda()
    A.check(L.pws_cvt_f32_to_bf16(A.ptr(d_src) if count else None, A.ptr(dst), count, acc, st), "cvt f32 -> bf16")
    torch.cuda.synchronize()
    got = dst.cpu()
    assert torch.equal(_bits16(got[count:]), _bits16(old[count:])), "written past count"
    want = ((old[:count].float() + src) if acc else src).bfloat16()
    g, w_ = got[:count].float(), want.float()
    nan = torch.isnan(w_)
    assert torch.equal(torch.isnan(g), nan)
    assert torch.equal(_bits16(got[:count])[~nan], _bits16(want)[~nan])
    # odd counts: the kernel converts pairs
    assert L.pws_cvt_f32_to_bf16(A.ptr(d_src) if count else A.ptr(dst), A.ptr(dst), count + 1, acc, st) == -22


# ------------------------------------------------------------------------------------------------------------ whole generator
def _make_net(kind, ngf, use_BN=False):
    from pwstablenet_amd.lib.networks_cascading import SingleDeviceParallel, UnetGenerator, define_G
    if use_BN:
        net = SingleDeviceParallel(UnetGenerator(31, 2, ngf, use_BN=True))
        sd = {"module." + k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_weights(kind, seed=123, ngf=ngf)}
        sd.update({"module." + k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_bn_state(seed=321, ngf=ngf)})
        net.load_state_dict(sd, strict=True)
        return net.cuda()
    net = define_G(31, 2, ngf, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights(kind, seed=123, ngf=ngf)})
    return net.cuda()


def _field_loss(grids, resid, tf):
    return sum(((g_ - tf) ** 2).mean() for g_ in grids) + 0.1 * sum((r * r).mean() for r in resid)


def _inputs(n):
    xw = torch.from_numpy(synth.make_window(n, 31, 256, seed=9))
    tfield = torch.from_numpy(np.random.RandomState(5).standard_normal((n, 256, 256, 2)).astype(np.float32)) * 0.3
    return xw, tfield


@pytest.fixture(scope="module")
def cpu_grad_ref17():
    """torch-CPU fp32 and float64 autograd of the restated graph (oracle/torch_ref.py, W1 weights, ngf 16) at n = 17, the field loss of
    test_hip_backward.test_netg_backward_vs_torch_cpu_autograd; computed once per module."""
    from oracle import torch_ref
    torch.set_num_threads(16)
    n = 17
    weights = synth.make_weights("W1", seed=123, ngf=16)
    xw, tfield = _inputs(n)
    out = []
    for dt in (torch.float32, torch.float64):
        ps = [torch.from_numpy(v).to(dt).requires_grad_(True) for _, v in weights]
        g, r = torch_ref.netg_forward(ps, xw.to(dt), True)
        loss = _field_loss(g, r, tfield.to(dt))
        loss.backward()
        out.append((loss.item(), [p.grad.numpy().astype(np.float64) for p in ps]))
    return weights, out[0], out[1]


def _step(net, x, tf):
    net.zero_grad()
    grids, resid = net(x)
    loss = _field_loss(grids, resid, tf)
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), [p.grad.clone() for p in net.module._ordered_params()]


@pytest.mark.parametrize("math,ngf", [("fp32", 16), ("bf16", 32)])
@pytest.mark.parametrize("n", [17, 32])
def test_deterministic_mode_at_training_batches(hip, cpu_grad_ref17, n, math, ngf):
    """At batches where the heads' backward slices (theta_bwd1_kernel: 2 / 4 sample slices; field_gz_kernel: 64 pixel slices per image):
    two deterministic runs are bit-identical, and the deterministic and default gradients agree within the atomics' noise.  fp32 at
    n = 17: both also lie within test_hip_backward's pinned per-tensor bound (_GRAD_TOL field/W1, product path: 1e-3) of the float64
    step [worst tensor 2.6e-4, as torch's own fp32 step is 8.3e-5 away]."""
    from test_hip_backward import _GRAD_TOL
    net = _make_net("W1", ngf)
    net.module.set_math(math)
    xw, tf = _inputs(n)
    x, tf = xw.cuda(), tf.cuda()
    free = _step(net, x, tf)
    net.module.deterministic = True
    a, b = _step(net, x, tf), _step(net, x, tf)
    net.module.deterministic = False
    assert a[0] == b[0]
    for ga, gb, gf in zip(a[1], b[1], free[1]):
        assert torch.equal(ga, gb)
        scale = float(gf.abs().max()) + 1e-12
        assert float((ga - gf).abs().max()) / scale < (1e-4 if math == "fp32" else 2e-2)
    if n != 17 or math != "fp32":
        return
    tol, cap = _GRAD_TOL[("field", "W1")][0]
    weights, (closs, cgrads), (dloss, dgrads) = cpu_grad_ref17
    for tag, (loss, grads) in (("deterministic", a), ("default", free)):
        assert abs(loss - dloss) < 1e-5 * max(1.0, abs(dloss))
        bad, rows = [], []
        for (name, _), got, ref, ref64 in zip(weights, grads, cgrads, dgrads):
            scale64 = max(np.abs(ref64).max(), 1e-12)
            e_cpu = np.abs(ref - ref64).max() / scale64
            e_hip = np.abs(got.cpu().numpy().astype(np.float64) - ref64).max() / scale64
            rows.append((e_hip, e_cpu, name))
            if not (e_hip < max(tol, 3 * e_cpu) and e_hip < cap):
                bad.append("%s: %.3g (torch fp32 %.3g; tol %.3g, cap %.3g)" % (name, e_hip, e_cpu, tol, cap))
        rows.sort(reverse=True)
        print("n=17 %s: worst tensors vs float64 (this path / torch fp32): %s" % (
            tag, "; ".join("%s %.2g/%.2g" % (nm, p, q) for p, q, nm in rows[:4])))
        assert not bad, tag + ":\n" + "\n".join(bad)


def test_use_bn_theta_head_gradients_at_a_sliced_batch(hip):
    """use_BN=True in train() mode at n = 32 (theta_bwd_bn_lin deals the samples to 4 slices): the theta head's parameter gradients
    (flatten / linear conv weights, their BatchNorms' gamma and beta) against torch-CPU float64 autograd of the restated graph
    (oracle/torch_ref.py with a BatchNorm after every conv), judged like test_hip_backward's whole-generator test: within `tol` of the
    float64 step or at most 3x as far as torch's own fp32 step, never beyond `cap`.  With 32 samples per channel the theta head's
    batch statistics are well conditioned (at n = 2 they divide by standard deviations near sqrt(eps)).  [worst tensor 3.6e-5 of its
    maximum against the bound 1e-3]"""
    from oracle import torch_ref
    from test_hip_backward import _GRAD_TOL
    tol, cap = _GRAD_TOL[("field", "W1")][0]
    n, ngf = 32, 16
    weights = synth.make_weights("W1", seed=123, ngf=ngf)
    bn_state = dict(synth.make_bn_state(seed=321, ngf=ngf))
    from pwstablenet_amd.spec import layer_specs
    specs = layer_specs(31, 2, ngf)
    xw, tfield = _inputs(n)
    net = _make_net("W1", ngf, use_BN=True).train()
    loss_hip, grads = _step(net, xw.cuda(), tfield.cuda())
    bns = net.module._bn_layers()
    torch.set_num_threads(16)
    ref = []
    for dt in (torch.float32, torch.float64):
        ps = [torch.from_numpy(v).to(dt).requires_grad_(True) for _, v in weights]
        bn = [tuple(torch.from_numpy(bn_state[ls.name[:-1] + "1." + k]).to(dt).requires_grad_(True) for k in ("weight", "bias")) for ls in specs]
        g, r = torch_ref.netg_forward(ps, xw.to(dt), True, bn=bn)
        loss = _field_loss(g, r, tfield.to(dt))
        loss.backward()
        ref.append((loss.item(), ps, bn))
    assert abs(loss_hip - ref[0][0]) < 1e-4 * max(1.0, abs(ref[0][0]))
    bad, rows = [], []
    for li, ls in enumerate(specs):
        if ls.name.split(".")[0] not in ("flatten", "linear"):
            continue
        # a conv bias in front of a BatchNorm has no gradient: this path writes exact zeros
        assert float(grads[2 * li + 1].abs().max()) == 0.0, ls.name
        cands = [(ls.name + ".weight", grads[2 * li], ref[0][1][2 * li], ref[1][1][2 * li]),
                 (ls.name[:-1] + "1.weight", bns[li].weight.grad, ref[0][2][li][0], ref[1][2][li][0]),
                 (ls.name[:-1] + "1.bias", bns[li].bias.grad, ref[0][2][li][1], ref[1][2][li][1])]
        for name, got, r32, r64 in cands:
            r64 = r64.grad.numpy()
            scale64 = max(np.abs(r64).max(), 1e-12)
            e_cpu = np.abs(r32.grad.numpy() - r64).max() / scale64
            e_hip = np.abs(got.cpu().numpy().astype(np.float64) - r64).max() / scale64
            rows.append((e_hip, e_cpu, name))
            if not (e_hip < max(tol, 3 * e_cpu) and e_hip < cap):
                bad.append("%s: %.3g (torch fp32 %.3g; tol %.3g, cap %.3g)" % (name, e_hip, e_cpu, tol, cap))
    print("use_BN n=32 theta head vs float64 (this path / torch fp32): %s" % "; ".join("%s %.2g/%.2g" % (nm, p, q) for p, q, nm in rows))
    assert not bad, "\n".join(bad)
