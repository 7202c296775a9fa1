"""CPU tests of tests/bn_ref.py, the float64 restatement tests/test_hip_bn_float64.py holds the BatchNorm training kernels to: against
torch's own float64 F.batch_norm + autograd, 1e-12 of each output's largest value; and the table of the generator's BatchNorm sites
the GPU test commits against pwstablenet_amd.spec."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as R  # noqa: E402

TOL = 1e-12
TORCH_ACT = {0: lambda t: t, 1: lambda t: F.leaky_relu(t, 0.2), 2: F.relu}


def _close(got, want, what, mag=None):
    err, mag = float((got - want).abs().max()), float(want.abs().max()) if mag is None else mag
    assert err <= TOL * mag, (what, err, mag)


@pytest.mark.parametrize("repeat", [1, 2])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("pixels,c", [(2, 3), (5, 1), (37, 6), (256, 2), (1000, 65)])
def test_restatement_equals_torch_float64(pixels, c, act, repeat):
    g = torch.Generator().manual_seed(1000 * pixels + 10 * c + act)
    z = torch.randn((pixels, c), generator=g, dtype=torch.float64) * (torch.rand(c, generator=g, dtype=torch.float64) * 1.5 + 0.5) \
        + torch.randn(c, generator=g, dtype=torch.float64) * 3
    gamma = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(c, generator=g, dtype=torch.float64) * 0.2
    rm0 = torch.randn(c, generator=g, dtype=torch.float64) * 0.1
    rv0 = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    dy = torch.randn((pixels, c), generator=g, dtype=torch.float64)
    eps, mom = 1e-5, 0.1
    # torch: the rows of (pixels, c) are the N * H * W positions of an NCHW tensor
    zt, gt, bt = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()
    for _ in range(repeat):     # a module called `repeat` times on the same input updates its running statistics every time
        yt = TORCH_ACT[act](F.batch_norm(zt.t().reshape(1, c, pixels), rm, rv, gt, bt, training=True, momentum=mom, eps=eps))
    yt.backward(dy.t().reshape(1, c, pixels))
    f = R.forward(z, gamma, beta, act, eps, mom, repeat, (rm0, rv0))
    _close(f["y"], yt.detach().reshape(c, pixels).t(), "y")
    _close(f["mean"], z.mean(0), "mean")
    _close(f["var"], z.var(0, unbiased=False), "var")
    _close(f["invstd"], 1 / torch.sqrt(z.var(0, unbiased=False) + eps), "invstd")
    _close(f["running_mean"], rm, "running_mean")
    _close(f["running_var"], rv, "running_var")
    f0 = R.forward(z, gamma, beta, act, eps, mom, 0, (rm0, rv0))              # repeat 0 leaves the running statistics alone
    assert torch.equal(f0["running_mean"], rm0) and torch.equal(f0["running_var"], rv0) and not torch.equal(f["running_mean"], rm0)
    b = R.backward(dy, f["y"] > 0, z, f["mean"], f["invstd"], gamma, act)
    # 2 pixels: xh = +-1 up to eps, the three terms of dz cancel to ~ eps / var of their size and leave their own float64 rounding
    # behind, in torch as here; dz is held to 1e-12 of its largest term there, of its own largest value everywhere else
    _close(b["dz"], zt.grad, "dz", float((gamma * f["invstd"] * dy).abs().max()) if pixels == 2 else None)
    _close(b["dgamma"], gt.grad, "dgamma")
    _close(b["dbeta"], bt.grad, "dbeta")


def test_without_running_statistics_and_without_mask():
    g = torch.Generator().manual_seed(5)
    z, dy = torch.randn((9, 4), generator=g), torch.randn((9, 4), generator=g)
    gamma, beta = torch.rand(4, generator=g) + 0.5, torch.randn(4, generator=g)
    f = R.forward(z, gamma, beta, 0, 1e-5)
    assert f["running_mean"] is None and f["running_var"] is None and f["y"].dtype == torch.float64
    a = R.backward(dy, None, z, f["mean"], f["invstd"], gamma, 0)
    b = R.backward(dy, f["y"] > 0, z, f["mean"], f["invstd"], gamma, 0)      # act 0: the mask does not matter
    assert all(torch.equal(a[k], b[k]) for k in a)
    # a constant channel: variance exactly 0, the finite invstd = 1 / sqrt(eps), y = act(beta)
    zc = torch.full((7, 2), 3.3)
    fc = R.forward(zc, gamma[:2], beta[:2], 1, 1e-5)
    assert float(fc["var"].abs().max()) == 0.0 and torch.equal(fc["invstd"], torch.full((2,), 1e-5, dtype=torch.float64).rsqrt())
    assert torch.equal(fc["y"], R.act64(beta[:2].double(), 1).expand(7, 2))


def test_native_batch_norm_is_what_f_batch_norm_computes():
    """The GPU test's fp32 yardstick calls torch.native_batch_norm (it returns the saved mean and invstd as well): the same bits as
    F.batch_norm, forward, running statistics and gradients."""
    g = torch.Generator().manual_seed(9)
    z, dy = torch.randn((1, 5, 301), generator=g) * 2 + 1, torch.randn((1, 5, 301), generator=g)
    outs = []
    for native in (False, True):
        zt, w, b = z.clone().requires_grad_(True), torch.full((5,), 1.25, requires_grad=True), torch.full((5,), -0.5, requires_grad=True)
        rm, rv = torch.zeros(5), torch.ones(5)
        y = torch.native_batch_norm(zt, w, b, rm, rv, True, 0.1, 1e-5)[0] if native else F.batch_norm(zt, rm, rv, w, b, True, 0.1, 1e-5)
        y.backward(dy)
        outs.append((y.detach(), rm, rv, zt.grad, w.grad, b.grad))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_committed_site_table_follows_the_spec():
    """The (pixels, c, act) of every BatchNorm the use_BN generator runs at n = 64 windows, ngf = 64, recomputed from the layer
    graph: a change of the architecture fails here until the table (and with it the GPU cases) follows."""
    import test_hip_bn_float64 as T
    assert sorted(T.sites_from_spec()) == sorted(T.SITES)
    assert sorted(T.site_cases()) == sorted(set((p, min(c, 65), a) for p, c, a in T.SITES))
