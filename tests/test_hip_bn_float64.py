"""The BatchNorm training kernels (pws_bn_train_fwd / pws_bn_train_bwd, csrc/bnorm.hip) against float64, at the pixel counts where the
reduction changes its walk, at the sites of the use_BN generator's training step, on ill-conditioned channels, and through every
argument variant the executor uses.

The reference is tests/bn_ref.py (float64, on the device, held to torch's float64 batch_norm by tests/test_bn_ref_cpu.py); it sees the
fp32 values the kernel sees.  The yardstick is torch's own fp32 batch_norm and its autograd on the same inputs (on the CPU, as
tests/test_hip_bn.py: torch.native_batch_norm, the operator under F.batch_norm, which also returns the saved mean and invstd), measured
against the same reference.  On every output

    kernel error  <=  4 x torch-fp32 error  +  4 fp32 ulps of the output's largest float64 magnitude          (max over the tensor)

Why 4: both sides evaluate the same fp32 formula in another summation order, torch's sums being the accurate end of what fp32 allows; one
more pass of roundings is legitimate, orders of magnitude are not.  The 4 ulps keep an output torch gets exactly from demanding equal
bits.  The backward's activation mask is the kernel's own forward y > 0 for the reference and for the yardstick, so a y within rounding
of 0 never enters and no element is left out.

Beside each bound, in brackets in the tests' docstrings: the largest kernel error / torch-fp32 error measured on an MI355X over the cases
of that test (cases where torch's error is 0 are held by the 4 ulps alone; the largest share of the bound used is given with them).
Before the statistics were taken around a pivot and summed in double the same tests measured, on the ill-conditioned channels, invstd
at 3.4e6 x (mean / std -1000) and 2.1e5 x (1000) torch's error, y 279 x, dz 353 x, dgamma 206 x, the constant channel's y 10.7 x (2.7 x
the bound), and at 2 pixels x 65 channels an invstd off by 1.1 absolute (1.4e5 x).
"""
import functools
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from pwstablenet_amd import spec  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

EPS, MOM = float(np.float32(1e-5)), float(np.float32(0.1))     # the fp32 values the kernel is handed
FACTOR, ULPS = 4.0, 4.0
NGF, NB, S = 64, 64, 256

# ------------------------------------------------------------------------------------------------------------ the generator's sites
# (pixels, c, act) of every BatchNorm of one use_BN step at n = 64 windows, ngf = 64 (stages run one by one: the statistics are per call);
# tests/test_bn_ref_cpu.py::test_committed_site_table_follows_the_spec recomputes it
SITES = [
    (64, 6, 1), (64, 512, 1),                                                      # the theta head: linear, flatten
    (256, 256, 1), (256, 256, 2),
    (1024, 256, 1), (1024, 256, 2), (1024, 512, 2),
    (4096, 256, 1), (4096, 256, 2), (4096, 512, 2),
    (16384, 256, 1), (16384, 256, 2), (16384, 512, 2),
    (65536, 256, 1), (65536, 256, 2), (65536, 512, 2),
    (262144, 128, 1), (262144, 128, 2), (262144, 256, 2),
    (1048576, 64, 1), (1048576, 64, 2), (1048576, 128, 2),
    (4194304, 2, 0), (4194304, 64, 1), (4194304, 64, 2),                           # the field head's BatchNorm(2), the first layer
]


def sites_from_spec(n=NB, ngf=NGF, side=S):
    """The table from the layer graph: encoder blocks (transfer, down*, down_bottom*) end in LeakyReLU, decoder blocks (up*, up_bottom*) in
    ReLU, the field head's BatchNorm has no activation of its own (netg_exec.h field()), the theta head normalises over the n samples."""
    out = set()
    for ls in spec.layer_specs(31, 2, ngf):
        block = ls.name.split(".")[0]
        lvl = int(re.sub(r"\D", "", block) or 0)
        if block in ("flatten", "linear"):
            out.add((n, ls.cout, 1))
            continue
        if block in ("transfer", "out"):
            h, act = side, 1 if block == "transfer" else 0
        elif block.startswith("down"):
            h, act = side >> (lvl - 1), 1
        else:
            h, act = side >> lvl, 2
        oh = (h + 2 * ls.p - ls.k) // ls.s + 1 if ls.kind == "conv" else (h - 1) * ls.s - 2 * ls.p + ls.k
        out.add((n * oh * oh, ls.cout, act))
    return sorted(out)


def site_cases():
    """The channel count changes blockIdx.y and the tail only (covered by CASES): min(c, 65) keeps every site's pixel count and activation."""
    return sorted(set((p, min(c, 65), a) for p, c, a in SITES))


# ------------------------------------------------------------------------------------------------------------ pixel x channel cases
# pixels: fewer than the 4 pixel lanes (2..5), one slab to two (255..257), 1023, the last uncapped count and the first capped one
# (262144, 262145), a capped ragged walk (262144 * 3 + 7), the first layer of a 64-window step (4194304).  channels: 1, 2, 63, 64, 65, 96,
# 512; 512 up to 1024 pixels, 65 up to 65536, 2 only above 262144 pixels.
CASES = [
    (2, 1, 0), (2, 64, 1), (2, 65, 1), (2, 512, 2),
    (3, 2, 1), (3, 63, 2), (3, 512, 0),
    (4, 1, 2), (4, 65, 0), (4, 96, 1),
    (5, 2, 0), (5, 64, 2), (5, 512, 1),
    (255, 1, 1), (255, 63, 0), (255, 65, 2), (255, 512, 1),
    (256, 2, 2), (256, 64, 1), (256, 96, 0),
    (257, 1, 0), (257, 65, 1), (257, 512, 2),
    (1023, 2, 1), (1023, 63, 2), (1023, 65, 0), (1023, 96, 0), (1023, 512, 1),
    (262144, 1, 1), (262144, 2, 0), (262144, 64, 1), (262144, 96, 2),
    (262145, 2, 0), (262145, 2, 1), (262145, 2, 2),
    (262144 * 3 + 7, 2, 1), (262144 * 3 + 7, 2, 2),
    (4194304, 2, 1), (4194304, 2, 2),
]


def ulp32(x):
    return float(np.spacing(np.float32(x)))


class Inputs:
    """Seeded fp32 inputs of one case, made on the device once; distinct per channel (own mean, spread, gamma, beta, running statistics
    and gradient scale)."""

    def __init__(self, pixels, c, seed=0, mean=None, std=None):
        g = torch.Generator(device="cuda").manual_seed(1_000_003 * seed + 7919 * (pixels % 1_000_003) + c)
        u = lambda lo, hi: torch.rand(c, device="cuda", generator=g) * (hi - lo) + lo     # noqa: E731
        self.pixels, self.c = pixels, c
        mean = u(-2, 2) if mean is None else torch.tensor(mean, device="cuda", dtype=torch.float32)
        std = u(0.5, 2) if std is None else torch.tensor(std, device="cuda", dtype=torch.float32)
        self.z = torch.randn((pixels, c), device="cuda", generator=g) * std + mean
        self.gamma, self.beta = u(0.5, 1.5), torch.randn(c, device="cuda", generator=g) * 0.2
        self.rm0, self.rv0 = torch.randn(c, device="cuda", generator=g) * 0.1, u(0.5, 1.5)
        self.dy = torch.randn((pixels, c), device="cuda", generator=g) * u(0.5, 2)


@functools.lru_cache(maxsize=1)
def inputs(pixels, c):
    return Inputs(pixels, c)


def kernel_fwd(A, z, gamma, beta, act, rm=None, rv=None, repeat=1, y=None, stats=None):
    L, c = A.lib(), z.shape[1]
    ws = torch.empty(L.pws_bn_ws_bytes(c), device="cuda", dtype=torch.uint8)
    y = torch.full_like(z, float("nan")) if y is None else y
    stats = torch.full((2 * c,), float("nan"), device="cuda") if stats is None else stats
    A.check(L.pws_bn_train_fwd(A.ptr(z), z.shape[0], c, A.ptr(gamma), A.ptr(beta), act, A.ptr(y), A.ptr(stats), A.ptr(rm), A.ptr(rv), MOM, EPS,
                               repeat, A.ptr(ws), ws.numel(), A.current_stream()), "bn fwd")
    return y, stats


def kernel_bwd(A, dy, y, z, stats, gamma, act, dgamma, dbeta):
    """dz is written over (a copy of) dy and returned."""
    L, c = A.lib(), z.shape[1]
    ws = torch.empty(L.pws_bn_ws_bytes(c), device="cuda", dtype=torch.uint8)
    dz = dy.clone()
    A.check(L.pws_bn_train_bwd(A.ptr(dz), A.ptr(y), A.ptr(z), A.ptr(stats), A.ptr(gamma), act, z.shape[0], c, A.ptr(dgamma), A.ptr(dbeta),
                               A.ptr(ws), ws.numel(), A.current_stream()), "bn bwd")
    return dz


def _rows(t):
    """(pixels, c) on the device -> torch's (1, c, pixels) on the CPU"""
    return t.t().contiguous().cpu().reshape(1, t.shape[1], t.shape[0])


def _cols(t, like):
    """torch's (1, c, pixels) on the CPU -> (pixels, c) on the device"""
    return t.reshape(like.shape[1], like.shape[0]).to(like.device).t()


class Torch32:
    """torch's fp32 batch_norm (+ its autograd) on the CPU on the same fp32 inputs."""

    def __init__(self, z, gamma, beta, act, rm0, rv0, repeat):
        self.like = z
        self.zt = _rows(z).requires_grad_(True)
        self.g, self.b = gamma.cpu().requires_grad_(True), beta.cpu().requires_grad_(True)
        self.rm, self.rv = rm0.cpu().clone(), rv0.cpu().clone()
        run = (self.rm, self.rv) if repeat else (None, None)     # repeat 0: no running statistics at all
        for _ in range(max(repeat, 1)):                          # a module called `repeat` times on the same input
            self.yb, mean, invstd = torch.native_batch_norm(self.zt, self.g, self.b, run[0], run[1], True, MOM, EPS)
        self.mean, self.invstd = mean.detach().to(z.device), invstd.detach().to(z.device)
        yb = _cols(self.yb.detach(), z)
        self.y = yb if act == 0 else torch.where(yb > 0, yb, yb * np.float32(R.SLOPE[act]))

    def backward(self, dyh):
        self.yb.backward(_rows(dyh))
        return _cols(self.zt.grad, self.like), self.g.grad.to(self.like.device), self.b.grad.to(self.like.device)


class Figures:
    """Every (output, kernel error, torch-fp32 error, bound) of a case: printed, then asserted together."""

    def __init__(self, what):
        self.what, self.rows = what, []

    def judge(self, name, got, ref, t32):
        assert bool(torch.isfinite(got).all()), (self.what, name, "not finite")
        ref = ref.double()
        ek, et, mag = float((got.double() - ref).abs().max()), float((t32.double() - ref).abs().max()), float(ref.abs().max())
        self.rows.append((name, ek, et, FACTOR * et + ULPS * ulp32(mag)))

    def judge_channels(self, name, got, ref, t32):
        """every channel an output of its own (channels of very different scale: the conditioning cases)"""
        for ch in range(ref.shape[-1]):
            self.judge("%s[ch %d]" % (name, ch), got[..., ch], ref[..., ch], t32[..., ch])

    def finish(self):
        bad = []
        for name, ek, et, bound in self.rows:
            ratio = ek / et if et > 0 else float("inf") if ek > 0 else 0.0
            print("%s %-18s kernel %.3e torch32 %.3e ratio %8.3f of-bound %.3f%s" % (self.what, name, ek, et, ratio, ek / bound,
                                                                                    "" if ek <= bound else "   <-- FAILS"))
            if not ek <= bound:
                bad.append((name, ek, et, bound))
        assert not bad, (self.what, bad)


def run_case(A, inp, act, tag, per_channel=False):
    """Forward and backward of one case through the kernels, the float64 reference and the fp32 yardstick; returns the Figures (not yet
    asserted) and what the kernels gave."""
    z, c = inp.z, inp.c
    fig = Figures("%s p=%d c=%d act=%d:" % (tag, inp.pixels, c, act))
    rm, rv = inp.rm0.clone(), inp.rv0.clone()
    y, stats = kernel_fwd(A, z, inp.gamma, inp.beta, act, rm, rv, 1)
    f = R.forward(z, inp.gamma, inp.beta, act, EPS, MOM, 1, (inp.rm0, inp.rv0))
    t = Torch32(z, inp.gamma, inp.beta, act, inp.rm0, inp.rv0, 1)
    fig.judge("y", y, f["y"], t.y)
    fig.judge("mean", stats[:c], f["mean"], t.mean)
    fig.judge("invstd", stats[c:], f["invstd"], t.invstd)
    fig.judge("running_mean", rm, f["running_mean"], t.rm.to(z.device))
    fig.judge("running_var", rv, f["running_var"], t.rv.to(z.device))
    if per_channel:
        fig.judge_channels("y", y, f["y"], t.y)
        fig.judge_channels("invstd", stats[c:], f["invstd"], t.invstd)
        fig.judge_channels("running_var", rv, f["running_var"], t.rv.to(z.device))
    # backward: the mask of the kernel's own forward for all three
    mask = y > 0
    dg0, db0 = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    dz = kernel_bwd(A, inp.dy, y, z, stats, inp.gamma, act, dg0, db0)
    b = R.backward(inp.dy, mask, z, f["mean"], f["invstd"], inp.gamma, act)
    dyh32 = inp.dy if act == 0 else torch.where(mask, inp.dy, inp.dy * np.float32(R.SLOPE[act]))
    tdz, tdg, tdb = t.backward(dyh32)
    fig.judge("dz", dz, b["dz"], tdz)
    fig.judge("dgamma", dg0, b["dgamma"], tdg)
    fig.judge("dbeta", db0, b["dbeta"], tdb)
    if per_channel:
        fig.judge_channels("dz", dz, b["dz"], tdz)
    return fig, {"y": y, "stats": stats, "rm": rm, "rv": rv, "dz": dz, "dgamma": dg0, "dbeta": db0, "ref": f}


@pytest.mark.parametrize("pixels,c,act", CASES)
def test_bn_vs_float64_at_the_walk_boundaries(hip, pixels, c, act):
    """y, mean, invstd, running statistics, dz, dgamma, dbeta within 4 x torch-fp32 error + 4 ulps.
    [y 2.52, mean 1.00, invstd 1.00, running_mean 4.10 (4 pixels, 0.25 of the bound), running_var 1.00, dz 1.58, dgamma 2.01, dbeta 1.00;
    largest share of a bound: y 0.47]"""
    fig, _ = run_case(hip, inputs(pixels, c), act, "walk")
    fig.finish()


@pytest.mark.parametrize("pixels,c,act", site_cases())
def test_bn_vs_float64_at_the_generators_sites(hip, pixels, c, act):
    """Every distinct (pixels, min(c, 65), act) of the use_BN generator's BatchNorms at n = 64, ngf = 64: the same outputs, the same bound.
    [y 1.67, mean 1.00, invstd 1.00, running_mean 1.27, running_var 1.04, dz 1.44, dgamma 1.15, dbeta 0.52; largest share of a bound: y 0.24]"""
    fig, _ = run_case(hip, inputs(pixels, c), act, "site")
    fig.finish()


# ------------------------------------------------------------------------------------------------------------ conditioning
RATIOS = [0.0, 1.0, -10.0, 100.0, -1000.0, 1000.0]     # mean / std of channels 0..5
STDS = [1.0, 2.0, 0.5, 1.5, 1.0, 0.25]
CONST = 3.3                                               # channel 6: the same value everywhere; channel 7: std 1e-3 around 0


@functools.lru_cache(maxsize=1)
def conditioning_inputs(pixels):
    mean = [r * s for r, s in zip(RATIOS, STDS)] + [CONST, 0.0]
    inp = Inputs(pixels, 8, seed=1, mean=mean, std=STDS + [0.0, 1e-3])
    assert bool((inp.z[:, 6] == np.float32(CONST)).all())
    return inp


@pytest.mark.parametrize("pixels,act", [(20000, 1), (20000, 0), (262145, 2)])
def test_bn_vs_float64_on_ill_conditioned_channels(hip, pixels, act):
    """Channels with mean / std of 0, 1, -10, 100, -1000, 1000 (a conv bias in front of the BatchNorm), one exactly constant channel
    (variance 0: invstd = 1 / sqrt(eps), y = act(beta)) and one of spread 1e-3 around 0: the bound of this file on the whole tensors and,
    for y, invstd, running_var and dz, on every channel as an output of its own.
    [whole tensors and single channels alike: y 0.22, mean 1.00, invstd 1.00, running_mean 1.00, running_var 1.22, dz 1.03, dgamma 0.98,
    dbeta 0.05; largest share of a bound: dgamma 0.25]"""
    inp = conditioning_inputs(pixels)
    fig, out = run_case(hip, inp, act, "cond", per_channel=True)
    fig.finish()
    want = R.act64(inp.beta[6].double(), act)
    assert float((out["y"][:, 6].double() - want).abs().max()) <= ULPS * ulp32(float(want.abs())), "constant channel: y != act(beta)"
    inv = float(out["stats"][8 + 6])
    assert np.isfinite(inv) and abs(inv - EPS ** -0.5) <= ULPS * ulp32(EPS ** -0.5), inv


# ------------------------------------------------------------------------------------------------------------ argument variants
VP, VC, VACT = 1023, 65, 1


def test_running_pointers_null_and_repeat(hip):
    """running_mean / running_var NULL: y and the saved statistics are those of the call that passes them, bit for bit.  repeat 0 / 1 / 3:
    the running statistics take that many updates (0: untouched), within the bound of this file.
    [running_mean 0.83, running_var 0.85; largest share of a bound 0.10]"""
    inp = inputs(VP, VC)
    rm, rv = inp.rm0.clone(), inp.rv0.clone()
    y1, s1 = kernel_fwd(hip, inp.z, inp.gamma, inp.beta, VACT, rm, rv, 1)
    y0, s0 = kernel_fwd(hip, inp.z, inp.gamma, inp.beta, VACT, None, None, 1)
    assert torch.equal(y0, y1) and torch.equal(s0, s1)
    for repeat in (0, 1, 3):
        rm, rv = inp.rm0.clone(), inp.rv0.clone()
        y, s = kernel_fwd(hip, inp.z, inp.gamma, inp.beta, VACT, rm, rv, repeat)
        assert torch.equal(y, y1) and torch.equal(s, s1)
        if repeat == 0:
            assert torch.equal(rm, inp.rm0) and torch.equal(rv, inp.rv0)
            continue
        f = R.forward(inp.z, inp.gamma, inp.beta, VACT, EPS, MOM, repeat, (inp.rm0, inp.rv0))
        t = Torch32(inp.z, inp.gamma, inp.beta, VACT, inp.rm0, inp.rv0, repeat)
        fig = Figures("variant repeat=%d:" % repeat)
        fig.judge("running_mean", rm, f["running_mean"], t.rm.cuda())
        fig.judge("running_var", rv, f["running_var"], t.rv.cuda())
        fig.finish()


def test_backward_variants(hip):
    """y = NULL with act = 0; dgamma / dbeta NULL (dz bit for bit that of the call that passes them); dgamma / dbeta accumulate onto what
    they hold.  [y = NULL: dz 0.98, dgamma 0.18, dbeta 0.07; largest share of a bound 0.11]"""
    inp = inputs(VP, VC)
    c = VC
    # y = NULL, act 0 (the field head's BatchNorm): same reference, same bound
    y, stats = kernel_fwd(hip, inp.z, inp.gamma, inp.beta, 0)
    f = R.forward(inp.z, inp.gamma, inp.beta, 0, EPS, MOM)
    t = Torch32(inp.z, inp.gamma, inp.beta, 0, inp.rm0, inp.rv0, 0)
    dg, db = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    dz = kernel_bwd(hip, inp.dy, None, inp.z, stats, inp.gamma, 0, dg, db)
    b = R.backward(inp.dy, None, inp.z, f["mean"], f["invstd"], inp.gamma, 0)
    tdz, tdg, tdb = t.backward(inp.dy)
    fig = Figures("variant y=NULL:")
    fig.judge("dz", dz, b["dz"], tdz), fig.judge("dgamma", dg, b["dgamma"], tdg), fig.judge("dbeta", db, b["dbeta"], tdb)
    fig.finish()
    dg2, db2 = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    assert torch.equal(kernel_bwd(hip, inp.dy, y, inp.z, stats, inp.gamma, 0, dg2, db2), dz) and torch.equal(dg2, dg) and torch.equal(db2, db)
    # with an activation: NULL dgamma / dbeta, and accumulation
    y, stats = kernel_fwd(hip, inp.z, inp.gamma, inp.beta, VACT)
    dg, db = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    dz = kernel_bwd(hip, inp.dy, y, inp.z, stats, inp.gamma, VACT, dg, db)
    for a, b_ in ((None, None), (dg.clone(), None), (None, db.clone())):
        assert torch.equal(kernel_bwd(hip, inp.dy, y, inp.z, stats, inp.gamma, VACT, a, b_), dz)
    g = torch.Generator(device="cuda").manual_seed(11)
    dg0, db0 = torch.randn(c, device="cuda", generator=g) * 50, torch.randn(c, device="cuda", generator=g) * 50
    dga, dba = dg0.clone(), db0.clone()
    assert torch.equal(kernel_bwd(hip, inp.dy, y, inp.z, stats, inp.gamma, VACT, dga, dba), dz)
    assert torch.equal(dga, dg0 + dg) and torch.equal(dba, db0 + db)      # one fp32 addition onto the contents
    assert not torch.equal(dga, dg)


def test_zero_pixels_writes_nothing(hip):
    """pixels == 0: both calls return OK and leave every buffer as it was (sentinels)."""
    L, c = hip.lib(), 5
    sent = lambda n: torch.full((n,), 123.5, device="cuda")     # noqa: E731
    z, y, stats, rm, rv, g, b, dg, db = sent(4 * c), sent(4 * c), sent(2 * c), sent(c), sent(c), sent(c), sent(c), sent(c), sent(c)
    ws = torch.full((L.pws_bn_ws_bytes(c) // 4,), 123.5, device="cuda")
    st = hip.current_stream()
    assert L.pws_bn_train_fwd(hip.ptr(z), 0, c, hip.ptr(g), hip.ptr(b), 1, hip.ptr(y), hip.ptr(stats), hip.ptr(rm), hip.ptr(rv), MOM, EPS, 1,
                              hip.ptr(ws), ws.numel() * 4, st) == 0
    assert L.pws_bn_train_bwd(hip.ptr(y), hip.ptr(y), hip.ptr(z), hip.ptr(stats), hip.ptr(g), 1, 0, c, hip.ptr(dg), hip.ptr(db), hip.ptr(ws),
                              ws.numel() * 4, st) == 0
    torch.cuda.synchronize()
    for t in (z, y, stats, rm, rv, g, b, dg, db, ws):
        assert bool((t == 123.5).all())


@pytest.mark.parametrize("pixels,c", [(VP, VC), (262144 * 3 + 7, 2)])
def test_two_calls_give_the_same_bits(hip, pixels, c):
    """The header of bnorm.hip promises determinism: forward and backward twice on the same inputs, every output bit for bit."""
    inp = inputs(pixels, c)
    outs = []
    for _ in range(2):
        rm, rv = inp.rm0.clone(), inp.rv0.clone()
        y, stats = kernel_fwd(hip, inp.z, inp.gamma, inp.beta, VACT, rm, rv, 1)
        dg, db = torch.ones(c, device="cuda"), torch.ones(c, device="cuda")
        dz = kernel_bwd(hip, inp.dy, y, inp.z, stats, inp.gamma, VACT, dg, db)
        outs.append((y, stats, rm, rv, dz, dg, db))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
