"""float64 restatement of training-mode BatchNorm + activation, forward and backward, from the formulas in the header of
pwstablenet_amd/csrc/bnorm.hip and torch's documentation of nn.BatchNorm2d (no F.batch_norm inside).  Plain torch on whatever device the
inputs live on; every input is converted to float64 first, so the reference sees exactly the values it is given.

Layout: z, dy, y are (pixels, c): row = one N * H * W position, column = channel (NHWC, as the kernels).  act: 0 none, 1 LeakyReLU(0.2),
2 ReLU (PWS_ACT_*).  tests/test_bn_ref_cpu.py holds this file to torch's own float64 batch_norm + autograd."""
import torch

SLOPE = {0: 1.0, 1: 0.2, 2: 0.0}   # the activation's slope where its output is not positive


def act64(t, act):
    return t if act == 0 else torch.where(t > 0, t, t * SLOPE[act])


def forward(z, gamma, beta, act, eps, momentum=0.1, repeat=1, running=None):
    """Returns a dict: mean, var (biased), invstd (c,), y (pixels, c), and running_mean / running_var (None without `running` =
    (running_mean, running_var)) after `repeat` updates r = (1 - momentum) r + momentum * (mean | unbiased variance)."""
    z = z.double()
    p = z.shape[0]
    mean = z.sum(0) / p
    d = z - mean
    var = (d * d).sum(0) / p
    invstd = 1.0 / torch.sqrt(var + eps)
    y = act64(gamma.double() * (d * invstd) + beta.double(), act)
    rm = rv = None
    if running is not None:
        rm, rv = running[0].double().clone(), running[1].double().clone()
        unbiased = var * p / (p - 1)
        for _ in range(repeat):
            rm = (1.0 - momentum) * rm + momentum * mean
            rv = (1.0 - momentum) * rv + momentum * unbiased
    return {"mean": mean, "var": var, "invstd": invstd, "y": y, "running_mean": rm, "running_var": rv}


def backward(dy, act_mask, z, mean, invstd, gamma, act=0):
    """dyh = dy * act' with act' = 1 where act_mask (the forward output was positive; None: everywhere) and the activation's slope elsewhere;
    returns a dict: dz (pixels, c), dgamma = sum dyh * xh, dbeta = sum dyh (c,)."""
    dy, z, mean, invstd, gamma = (t.double() for t in (dy, z, mean, invstd, gamma))
    p = z.shape[0]
    dyh = dy if (act == 0 or act_mask is None) else torch.where(act_mask, dy, dy * SLOPE[act])
    xh = (z - mean) * invstd
    dgamma = (dyh * xh).sum(0)
    dbeta = dyh.sum(0)
    dz = gamma * invstd * (dyh - dbeta / p - xh * (dgamma / p))
    return {"dz": dz, "dgamma": dgamma, "dbeta": dbeta}
