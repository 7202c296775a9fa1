"""The VGG-16 perceptual term (pwstablenet_amd/perceptual.py, csrc/pool.hip and the conv kernels) at the batch of a training step
(bench.py's with_vgg leg: 64 images at 256 x 256), against float64.

1. The launch table.  VGG16Features(math) forward + backward on 64 images under the profiler, fp32 and bf16 math: every launch
   gives (pass, op, kernel, N, math).  N is the record's flops over the op's flops per sample.  TABLE below is that list in launch
   order, committed; test_live_launch_table_equals_the_committed_one recomputes it, so a dispatch change fails there until the
   table is updated.  ODD_TABLE is the same at n = 33 for the ops on 32 x 32 and 16 x 16 maps: the 16-wide Winograd ring pairs two
   samples per unit (conv_wring.hip g16: w == 16 and n even), an odd batch runs something else.  The profiler names kernel
   families; the pools are "objective_kernels" (KID_OBJECTIVE).
2. Every entry of the tables through the C ABI, exactly as _VGGFn drives it: the packs of VGG16Features._packed_weights(math), the
   padded NHWC input of pws_nchw_to_nhwc_pad_s, ACT_RELU and the store mode; in fp32 pws_act_bwd_bias_s before each data
   gradient, in bf16 the fused act_y / relu_mask wherever _VGGFn.backward sets them.  Each op's input is the HIP chain's own
   activation and each backward op's upstream gradient the chain's own gradient, so errors do not compound and ReLU masks and
   argmax windows are those of the chain.  The profiler must show the table's kernel for every call.  The reference is torch in
   float64 on the device (cudnn / MIOpen off: torch's own im2col + GEMM) over the whole batch and every channel, in chunks of
   samples.  bf16: the weights are rounded once (the packs' rounding is checked to be torch's), the chain's activations and
   gradients are bf16 already.  Max-pool forward and backward and the act' pass are bit-equal to float64.
3. The MSE kernels (pws_sqdiff_sum / pws_sqdiff_bwd) at counts below, at and above the sum's 2048-workgroup cap, and the
   perceptual term of a training step (3 stages x 64 fakes + 64 stable frames) against the float64 oracle chain.

Bounds are relative to the tensor's largest float64 value, with the largest error measured on an MI355X in brackets.  They are
those of tests/test_hip_train_batches.py (themselves within tests/test_hip_sweep.py / tests/test_hip_bf16.py) or tighter.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

NB, N_ODD, S = 64, 33, 256          # the step's batch, an odd batch, the image side
SEED_W = 13                          # VGG16Features.init_random seed
CPAD = {"fp32": 16, "bf16": 32}      # the RGB input zero-padded to the channels the conv kernels take

FWD_TOL = {"fp32": 5e-6,    # [1.1e-6]  Winograd transforms and K chunks in fp32 (test_hip_train_batches FWD_TOL: 2e-5)
           "bf16": 6e-3}    # [3.4e-3]  one bf16 rounding of the result: <= 2^-8 of the value (test_hip_sweep TOL)
DGRAD_TOL = {"fp32": 1e-5,  # [2.3e-6]  the direct kernel, sums of 9 x cout products (test_hip_train_batches DGRAD_TOL: 2e-5)
             "bf16": 6e-3}  # [3.5e-3]  act' of act_y and the bf16 rounding of the sum (test_hip_sweep TOL)


def _ops():
    """[(name, kind 'conv' | 'pool', cin, cout, input side)] in forward order (perceptual.VGG16_CFG at 256 x 256)."""
    from pwstablenet_amd.perceptual import VGG16_CFG
    out, cin, h, blk, k = [], 3, S, 1, 1
    for v in VGG16_CFG:
        if v == "M":
            out.append(("pool%d" % blk, "pool", cin, cin, h))
            h, blk, k = h // 2, blk + 1, 1
        else:
            out.append(("conv%d_%d" % (blk, k), "conv", cin, v, h))
            cin, k = v, k + 1
    return out


OPS = _ops()
OP = {o[0]: o for o in OPS}
CONVS = [o[0] for o in OPS if o[1] == "conv"]


def _per_sample_flops(pas, name, math):
    """What the launcher records per sample (conv_mfma.hip info(), pool.hip / conv_wgrad.hip ProfScope)."""
    _, kind, cin, cout, h = OP[name]
    if kind == "pool":
        return (3.0 if pas == "fwd" else 8.0) * (h // 2) * (h // 2) * cin
    if pas == "act":
        return 2.0 * h * h * cout
    cin = CPAD[math] if cin == 3 else cin
    return 2.0 * h * h * cout * cin * 9


# ------------------------------------------------------------------------------------------------------------ the committed tables
# (pass, op, kernel, N, math) in launch order of one forward + backward at n = 64 (test_live_launch_table_equals_the_committed_one)
TABLE = [
    ('fwd', 'conv1_1', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'conv1_2', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'pool1', 'objective_kernels', 64, 'bf16'),
    ('fwd', 'conv2_1', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'conv2_2', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'pool2', 'objective_kernels', 64, 'bf16'),
    ('fwd', 'conv3_1', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'conv3_2', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'conv3_3', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'pool3', 'objective_kernels', 64, 'bf16'),
    ('fwd', 'conv4_1', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'conv4_2', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'conv4_3', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'pool4', 'objective_kernels', 64, 'bf16'),
    ('fwd', 'conv5_1', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'conv5_2', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'conv5_3', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'pool5', 'objective_kernels', 64, 'bf16'),
    ('bwd', 'pool5', 'objective_kernels', 64, 'bf16'),
    ('dgrad', 'conv5_3', 'conv_ring_kernel', 64, 'bf16'),
    ('dgrad', 'conv5_2', 'conv_ring_kernel', 64, 'bf16'),
    ('dgrad', 'conv5_1', 'conv_ring_kernel', 64, 'bf16'),
    ('bwd', 'pool4', 'objective_kernels', 64, 'bf16'),
    ('dgrad', 'conv4_3', 'conv_ring_kernel', 64, 'bf16'),
    ('dgrad', 'conv4_2', 'conv_ring_kernel', 64, 'bf16'),
    ('dgrad', 'conv4_1', 'conv_ring_kernel', 64, 'bf16'),
    ('bwd', 'pool3', 'objective_kernels', 64, 'bf16'),
    ('dgrad', 'conv3_3', 'conv_ring_kernel', 64, 'bf16'),
    ('dgrad', 'conv3_2', 'conv_ring_kernel', 64, 'bf16'),
    ('dgrad', 'conv3_1', 'conv_ring_kernel', 64, 'bf16'),
    ('bwd', 'pool2', 'objective_kernels', 64, 'bf16'),
    ('dgrad', 'conv2_2', 'conv_ring_kernel', 64, 'bf16'),
    ('dgrad', 'conv2_1', 'conv_ring_kernel', 64, 'bf16'),
    ('bwd', 'pool1', 'objective_kernels', 64, 'bf16'),
    ('dgrad', 'conv1_2', 'conv_ring_kernel', 64, 'bf16'),
    ('dgrad', 'conv1_1', 'conv_ring_kernel', 64, 'bf16'),
    ('fwd', 'conv1_1', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'conv1_2', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'pool1', 'objective_kernels', 64, 'fp32'),
    ('fwd', 'conv2_1', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'conv2_2', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'pool2', 'objective_kernels', 64, 'fp32'),
    ('fwd', 'conv3_1', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'conv3_2', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'conv3_3', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'pool3', 'objective_kernels', 64, 'fp32'),
    ('fwd', 'conv4_1', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'conv4_2', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'conv4_3', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'pool4', 'objective_kernels', 64, 'fp32'),
    ('fwd', 'conv5_1', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'conv5_2', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'conv5_3', 'wino_ring_kernel<F(2x2,3x3)>', 64, 'fp32'),
    ('fwd', 'pool5', 'objective_kernels', 64, 'fp32'),
    ('bwd', 'pool5', 'objective_kernels', 64, 'fp32'),
    ('act', 'conv5_3', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv5_3', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
    ('act', 'conv5_2', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv5_2', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
    ('act', 'conv5_1', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv5_1', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
    ('bwd', 'pool4', 'objective_kernels', 64, 'fp32'),
    ('act', 'conv4_3', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv4_3', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
    ('act', 'conv4_2', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv4_2', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
    ('act', 'conv4_1', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv4_1', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
    ('bwd', 'pool3', 'objective_kernels', 64, 'fp32'),
    ('act', 'conv3_3', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv3_3', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
    ('act', 'conv3_2', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv3_2', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
    ('act', 'conv3_1', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv3_1', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
    ('bwd', 'pool2', 'objective_kernels', 64, 'fp32'),
    ('act', 'conv2_2', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv2_2', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
    ('act', 'conv2_1', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv2_1', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
    ('bwd', 'pool1', 'objective_kernels', 64, 'fp32'),
    ('act', 'conv1_2', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv1_2', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
    ('act', 'conv1_1', 'act_bwd_bias_kernel', 64, 'fp32'),
    ('dgrad', 'conv1_1', 'conv_mfma_kernel<k3s1,16x16>', 64, 'fp32'),
]

# the same at n = 33, ops on 32 x 32 and 16 x 16 input maps only
ODD_TABLE = [
    ('fwd', 'conv4_1', 'conv_ring_kernel', 33, 'bf16'),
    ('fwd', 'conv4_2', 'conv_ring_kernel', 33, 'bf16'),
    ('fwd', 'conv4_3', 'conv_ring_kernel', 33, 'bf16'),
    ('fwd', 'pool4', 'objective_kernels', 33, 'bf16'),
    ('fwd', 'conv5_1', 'conv_ring_kernel', 33, 'bf16'),
    ('fwd', 'conv5_2', 'conv_ring_kernel', 33, 'bf16'),
    ('fwd', 'conv5_3', 'conv_ring_kernel', 33, 'bf16'),
    ('fwd', 'pool5', 'objective_kernels', 33, 'bf16'),
    ('bwd', 'pool5', 'objective_kernels', 33, 'bf16'),
    ('dgrad', 'conv5_3', 'conv_ring_kernel', 33, 'bf16'),
    ('dgrad', 'conv5_2', 'conv_ring_kernel', 33, 'bf16'),
    ('dgrad', 'conv5_1', 'conv_ring_kernel', 33, 'bf16'),
    ('bwd', 'pool4', 'objective_kernels', 33, 'bf16'),
    ('dgrad', 'conv4_3', 'conv_ring_kernel', 33, 'bf16'),
    ('dgrad', 'conv4_2', 'conv_ring_kernel', 33, 'bf16'),
    ('dgrad', 'conv4_1', 'conv_ring_kernel', 33, 'bf16'),
    ('fwd', 'conv4_1', 'wino_ring_kernel<F(2x2,3x3)>', 33, 'fp32'),
    ('fwd', 'conv4_2', 'wino_ring_kernel<F(2x2,3x3)>', 33, 'fp32'),
    ('fwd', 'conv4_3', 'wino_ring_kernel<F(2x2,3x3)>', 33, 'fp32'),
    ('fwd', 'pool4', 'objective_kernels', 33, 'fp32'),
    ('fwd', 'conv5_1', 'wino_k3s1_kernel<F(2x2,3x3)>', 33, 'fp32'),
    ('fwd', 'conv5_2', 'wino_k3s1_kernel<F(2x2,3x3)>', 33, 'fp32'),
    ('fwd', 'conv5_3', 'wino_k3s1_kernel<F(2x2,3x3)>', 33, 'fp32'),
    ('fwd', 'pool5', 'objective_kernels', 33, 'fp32'),
    ('bwd', 'pool5', 'objective_kernels', 33, 'fp32'),
    ('act', 'conv5_3', 'act_bwd_bias_kernel', 33, 'fp32'),
    ('dgrad', 'conv5_3', 'conv_mfma_kernel<k3s1,16x16>', 33, 'fp32'),
    ('act', 'conv5_2', 'act_bwd_bias_kernel', 33, 'fp32'),
    ('dgrad', 'conv5_2', 'conv_mfma_kernel<k3s1,16x16>', 33, 'fp32'),
    ('act', 'conv5_1', 'act_bwd_bias_kernel', 33, 'fp32'),
    ('dgrad', 'conv5_1', 'conv_mfma_kernel<k3s1,16x16>', 33, 'fp32'),
    ('bwd', 'pool4', 'objective_kernels', 33, 'fp32'),
    ('act', 'conv4_3', 'act_bwd_bias_kernel', 33, 'fp32'),
    ('dgrad', 'conv4_3', 'conv_mfma_kernel<k3s1,16x16>', 33, 'fp32'),
    ('act', 'conv4_2', 'act_bwd_bias_kernel', 33, 'fp32'),
    ('dgrad', 'conv4_2', 'conv_mfma_kernel<k3s1,16x16>', 33, 'fp32'),
    ('act', 'conv4_1', 'act_bwd_bias_kernel', 33, 'fp32'),
    ('dgrad', 'conv4_1', 'conv_mfma_kernel<k3s1,16x16>', 33, 'fp32'),
]


def _vgg(math):
    from pwstablenet_amd.perceptual import VGG16Features
    return VGG16Features(math).init_random(SEED_W).cuda()


def _images(n, seed):
    """synth frames scaled to [-1, 1], as the warped frames are (distinct per sample)."""
    return torch.from_numpy(synth.make_frames(n, 3, S, S, seed=seed) / 127.5 - 1).float().cuda()


def _feature_grad(n, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(977 + n)
    return torch.randn((n, S // 32, S // 32, 512), device="cuda", generator=g).to(dtype)


def _odd_op(name):
    return OP[name][4] <= 32


def _label(recs, seq, math, n):
    """[(pass, op, kernel, N, math)] of the records of one forward (seq = forward ops) or backward (seq = reversed ops)."""
    out, i = [], 0
    for name, _tag, flops, _, _ in recs:
        assert i < len(seq), ("more launches than ops", name)
        op, kind = seq[i][0], seq[i][1]
        if name == "act_bwd_bias_kernel":
            pas = "act"
        else:
            pas = "fwd" if seq is OPS else ("bwd" if kind == "pool" else "dgrad")
            i += 1
        per = _per_sample_flops(pas, op, math)
        nn_ = int(round(flops / per))
        assert nn_ * per == flops and nn_ == n, (name, op, pas, flops, per, n)
        out.append((pas, op, name, nn_, math))
    assert i == len(seq), ("fewer launches than ops", i, len(seq))
    return out


def live_table(hip, math, n):
    """The launch table of VGG16Features(math) forward + backward on n images (module path, not the C ABI replay below)."""
    A = hip
    L = A.lib()
    net = _vgg(math)
    x = _images(n, 5).requires_grad_(True)
    gf = _feature_grad(n)
    L.pws_prof_enable(1)
    try:
        f = net(x)
        torch.cuda.synchronize()
        fwd = A.prof_collect()
        f.backward(gf)
        torch.cuda.synchronize()
        bwd = A.prof_collect()
    finally:
        L.pws_prof_enable(0)
    table = _label(fwd, OPS, math, n) + _label(bwd, OPS[::-1], math, n)
    return table, f.detach(), x.grad


def _want_table(math, odd):
    if odd:
        return [e for e in ODD_TABLE if e[4] == math]
    return [e for e in TABLE if e[4] == math]


@pytest.mark.parametrize("odd", [False, True], ids=["N64", "N33"])
@pytest.mark.parametrize("math", ["fp32", "bf16"])
def test_live_launch_table_equals_the_committed_one(hip, math, odd):
    """The tripwire: a dispatch change at the training batch (or at the odd batch on the deep maps) fails here until the tables
    and with them the cases below follow it.  Every op has its passes: forward, data gradient (fp32: with its act' pass), pool
    backward."""
    n = N_ODD if odd else NB
    live, _, _ = live_table(hip, math, n)
    if odd:
        live = [e for e in live if _odd_op(e[1])]
    print("%s n=%d live table:\n%s" % (math, n, "\n".join("    %r," % (e,) for e in live)))
    want = _want_table(math, odd)
    assert live == want, "launch table changed:\n  gone: %s\n  new:  %s" % (
        [e for e in want if e not in live], [e for e in live if e not in want])
    for name, kind, _, _, _ in OPS:
        if odd and not _odd_op(name):
            continue
        passes = sorted(e[0] for e in live if e[1] == name)
        if kind == "pool":
            assert passes == ["bwd", "fwd"], (name, passes)
        else:
            assert passes == (["act", "dgrad", "fwd"] if math == "fp32" else ["dgrad", "fwd"]), (name, passes)


# ------------------------------------------------------------------------------------------------------------ the C ABI chain
def _profiled(A, fn):
    L = A.lib()
    L.pws_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.pws_prof_enable(0)
    return A.prof_collect()


class _Chain:
    """One VGG16Features(math) forward + backward on n images through the C ABI, call for call as _VGGFn (perceptual.py), keeping
    every activation, every gradient and each call's profiler records: fwd[op] = (input, output, recs); bwd[op] = (upstream
    gradient, gradient after act' (fp32 conv: pws_act_bwd_bias_s), result, fused act' / relu_mask, act recs, recs).  The images
    are the plain synth frames: flat over about 11 % of their 2 x 2 windows, so the max-pool checks meet exact ties."""

    def __init__(self, A, math, n):
        L, st = A.lib(), A.current_stream()
        self.math, self.n = math, n
        net = self.net = _vgg(math)
        s16 = math == "bf16"
        store, dt, cpad = (A.STORE_BF16, torch.bfloat16, 32) if s16 else (A.STORE_FP32, torch.float32, 16)
        self.x = _images(n, 5)
        cur = torch.empty((n, S, S, cpad), device="cuda", dtype=dt)
        A.check(L.pws_nchw_to_nhwc_pad_s(A.ptr(self.x), A.ptr(cur), n, 3, S, S, cpad, store, st), "pws_nchw_to_nhwc_pad_s")
        self.xpad = cur
        packs = self.packs = net._packed_weights(math)
        self.fwd, self.bwd = {}, {}
        order = []
        ci = 0
        for name, kind, cin, cout, h in OPS:
            if kind == "pool":
                out = torch.empty((n, h // 2, h // 2, cur.shape[3]), device="cuda", dtype=dt)
                fn = lambda: A.check(L.pws_maxpool2x2_fwd_s(A.ptr(cur), A.ptr(out), n, h, h, cur.shape[3], store, st), "pool fwd")  # noqa: E731
            else:
                pk = packs[ci]
                out = torch.empty((n, h, h, cout), device="cuda", dtype=dt)
                a = A.PwsConvArgs()
                a.kind, a.n, a.h, a.w, a.nsrc = A.CONV_K3S1, n, h, h, 1
                a.src[0].ptr, a.src[0].channels, a.src[0].ld = cur.data_ptr(), cur.shape[3], cur.shape[3]
                a.cout, a.w_packed, a.bias, a.act = cout, pk["w"].data_ptr(), pk["b"].data_ptr(), A.ACT_RELU
                a.out, a.out_ld = out.data_ptr(), cout
                a.w_wino = pk["wino"].data_ptr()
                if pk["wring"] is not None:
                    a.w_wring = pk["wring"].data_ptr()
                if s16:
                    a.math, a.w_bf16, a.store = A.MATH_BF16, pk["bf16"].data_ptr(), A.STORE_BF16
                fn = lambda: A.check(L.pws_conv2d_fwd(ctypes.byref(a), st), "pws_conv2d_fwd")  # noqa: E731
                ci += 1
            self.fwd[name] = (cur, out, _profiled(A, fn))
            order.append((name, kind, cur, out))
            cur = out
        self.gfeat = _feature_grad(n)
        if s16:
            g = torch.empty(self.gfeat.shape, device="cuda", dtype=torch.bfloat16)
            A.check(L.pws_cvt_f32_to_bf16(A.ptr(self.gfeat), A.ptr(g), g.numel(), 0, st), "pws_cvt_f32_to_bf16")
            self.gfeat16 = g
        else:
            g = self.gfeat.clone()
        masked = False
        ra = order[::-1]
        for idx, (name, kind, xin, out) in enumerate(ra):
            h = xin.shape[1]
            prev_is_conv = idx + 1 < len(ra) and ra[idx + 1][1] == "conv"
            fuse = s16 and prev_is_conv
            dx = torch.empty_like(xin)
            gm, recs_act = g, []
            if kind == "pool":
                fn = lambda: A.check(L.pws_maxpool2x2_bwd_s(A.ptr(xin), A.ptr(g), A.ptr(dx), n, h, h, xin.shape[3], store,  # noqa: E731
                                                            1 if fuse else 0, st), "pool bwd")
            else:
                pk = packs[CONVS.index(name)]
                cout = out.shape[3]
                if not masked:   # the act' pass works in place: on a copy here, g is the previous op's result and kept for its check
                    gm = g.clone()
                    recs_act = _profiled(A, lambda: A.check(L.pws_act_bwd_bias_s(A.ptr(gm), A.ptr(out), n * h * h, cout, A.ACT_RELU,
                                                                                 None, store, None, 0, st), "pws_act_bwd_bias_s"))
                d = A.PwsConvBwdDataArgs()
                d.kind, d.n, d.h, d.w, d.cout = A.CONV_K3S1, n, h, h, cout
                d.gout, d.gout_ld, d.w_dgrad, d.ndst = gm.data_ptr(), cout, pk["dg"].data_ptr(), 1
                d.dst[0].ptr, d.dst[0].channels, d.dst[0].ld, d.dst[0].accumulate = dx.data_ptr(), xin.shape[3], xin.shape[3], 0
                if fuse:
                    d.dst[0].act_y, d.dst[0].act_y_ld, d.dst[0].act = xin.data_ptr(), xin.shape[3], A.ACT_RELU
                if s16:
                    d.math, d.w_dgrad_bf16, d.store = A.MATH_BF16, pk["dg_bf16"].data_ptr(), store
                fn = lambda: A.check(L.pws_conv2d_bwd_data(ctypes.byref(d), st), "pws_conv2d_bwd_data")  # noqa: E731
            recs = _profiled(A, fn)
            self.bwd[name] = (g, gm, dx, fuse, recs_act, recs)
            masked = fuse
            g = dx
        self.dx = g


_chains = {}


def _chain(A, math, n):
    key = (math, n)
    if key not in _chains:
        while len(_chains) >= 2:   # two chains at a time (the cases are grouped by math and batch below)
            _chains.pop(next(iter(_chains)))
        _chains[key] = _Chain(A, math, n)
    else:
        _chains[key] = _chains.pop(key)   # most recently used last
    return _chains[key]


@pytest.mark.parametrize("math", ["fp32", "bf16"])
def test_chain_replays_the_module_and_the_packs_round_as_torch(hip, math):
    """The chain is _VGGFn call for call: same features and input gradient as VGG16Features on the same images, weights and
    feature gradient.  Its operands: the padded input is the images (bf16: torch's rounding of them) with zero padding channels;
    the packs hold the module's weights -- fp32 pack unpacked equal, bf16 packs equal to torch's RNE rounding of the fp32 packs,
    the data-gradient pack a permutation of the weights; the bf16 feature gradient is torch's rounding of the fp32 one."""
    A = hip
    L, st = A.lib(), A.current_stream()
    ch = _chain(A, math, NB)
    _, f_mod, dx_mod = live_table(A, math, NB)
    feat = ch.fwd["pool5"][1].float()
    dx = ch.dx.float()[..., :3].permute(0, 3, 1, 2)
    ef = float((feat - f_mod).abs().max()) / float(f_mod.abs().max())
    ed = float((dx - dx_mod).abs().max()) / float(dx_mod.abs().max())
    print("%s chain vs module: features %.3g, input gradient %.3g (relative max)" % (math, ef, ed))
    assert ef <= 1e-6 and ed <= 1e-6, (ef, ed)   # [0 and 0: bit-equal]
    bf = math == "bf16"
    cpad = CPAD[math]
    xn = ch.x.permute(0, 2, 3, 1)
    assert torch.equal(ch.xpad[..., :3], xn.bfloat16() if bf else xn)
    assert float(ch.xpad[..., 3:].float().abs().max()) == 0.0
    if bf:
        assert torch.equal(ch.gfeat16, ch.gfeat.bfloat16())
    for m, pk in zip(ch.net._convs(), ch.packs):
        cin, cout = m.in_channels, m.out_channels
        w = m.weight.detach()
        if cin == 3:
            w = torch.cat([w, torch.zeros((cout, cpad - 3, 3, 3), device="cuda")], 1)
            cin = cpad
        wu = torch.empty_like(w)
        A.check(L.pws_unpack_conv_weight(A.ptr(pk["w"]), A.ptr(wu), A.CONV_K3S1, cin, cout, st), "unpack")
        torch.cuda.synchronize()
        assert torch.equal(wu, w)
        assert torch.equal(pk["b"], m.bias.detach())
        assert pk["dg"].numel() == 9 * cin * cout
        assert torch.equal(pk["dg"].sort().values, w.flatten().sort().values)
        if bf:
            # pack_bf16_kernel: [plane][npad][kpad] bf16 from the fp32 [plane][krows][ncols]
            for src, wb, kr, nc in ((pk["w"], pk["bf16"], cin, cout), (pk["dg"], pk["dg_bf16"], cout, cin)):
                kpad, npad = (kr + 31) // 32 * 32, (nc + 63) // 64 * 64
                got = wb.view(torch.bfloat16).view(9, npad, kpad)
                want = src[:9 * kr * nc].view(9, kr, nc).transpose(1, 2).bfloat16()
                assert torch.equal(got[:, :nc, :kr], want)
                assert float(got[:, nc:].float().abs().max() if npad > nc else 0.0) == 0.0
                assert float(got[:, :, kr:].float().abs().max() if kpad > kr else 0.0) == 0.0


# ------------------------------------------------------------------------------------------------------------ per-entry checks
class _Err:
    def __init__(self):
        self.num, self.den = 0.0, 0.0

    def add(self, got, want):
        self.num = max(self.num, float((got.double() - want).abs().max()))
        self.den = max(self.den, float(want.abs().max()))

    @property
    def rel(self):
        return self.num / max(self.den, 1e-30)


def _chunk(n, per_sample_elems):
    return max(1, min(n, int((1 << 27) // max(per_sample_elems, 1))))   # ~1 GB of float64 per operand


def _nchw64(t):
    return t.permute(0, 3, 1, 2).double()


def _w64(ch, name):
    """The float64 weights the chain's packs hold: RGB input channels zero-padded; bf16 math: rounded once (RNE)."""
    m = ch.net._convs()[CONVS.index(name)]
    w = m.weight.detach()
    if w.shape[1] == 3:
        w = torch.cat([w, torch.zeros((w.shape[0], CPAD[ch.math] - 3, 3, 3), device="cuda")], 1)
    return (w.bfloat16() if ch.math == "bf16" else w).double(), m.bias.detach().double()


def _expect(recs, kernel, pas, name, n, math):
    names = [r[0] for r in recs]
    assert names == [kernel], (names, kernel)
    per = _per_sample_flops(pas, name, math)
    assert recs[0][2] == per * n, (recs[0][2], per * n)


def check_conv_fwd(ch, name):
    xin, out, _ = ch.fwd[name]
    w64, b64 = _w64(ch, name)
    n, h = ch.n, xin.shape[1]
    err = _Err()
    step = _chunk(n, max(xin.shape[3], out.shape[3]) * h * h * 2)
    with torch.backends.cudnn.flags(enabled=False):
        for s0 in range(0, n, step):
            s = slice(s0, min(n, s0 + step))
            want = F.relu(F.conv2d(_nchw64(xin[s]), w64, b64, padding=1)).permute(0, 2, 3, 1)
            err.add(out[s], want)
    assert not torch.isnan(out).any()
    return err.rel


def check_conv_dgrad(ch, name):
    xin, out, _ = ch.fwd[name]
    _, g, dx, fuse, _, _ = ch.bwd[name]
    w64, _ = _w64(ch, name)
    n, h = ch.n, xin.shape[1]
    err = _Err()
    step = _chunk(n, max(xin.shape[3], out.shape[3]) * h * h * 3)
    with torch.backends.cudnn.flags(enabled=False):
        for s0 in range(0, n, step):
            s = slice(s0, min(n, s0 + step))
            want = F.conv_transpose2d(_nchw64(g[s]), w64, padding=1).permute(0, 2, 3, 1)   # d conv2d(x, w, padding=1) / dx
            if fuse:
                want = want * (xin[s] > 0)
            err.add(dx[s], want)
    assert not torch.isnan(dx).any()
    return err.rel


def check_act(ch, name):
    """fp32: pws_act_bwd_bias_s(ACT_RELU) multiplies the upstream gradient by (y > 0): a selection, exact."""
    _, out, _ = ch.fwd[name]
    gin, gm, _, _, _, _ = ch.bwd[name]
    assert torch.equal(gm, gin * (out > 0))


def check_pool_fwd(ch, name):
    xin, out, _ = ch.fwd[name]
    n = ch.n
    step = _chunk(n, xin[0].numel())
    for s0 in range(0, n, step):
        s = slice(s0, min(n, s0 + step))
        want = F.max_pool2d(_nchw64(xin[s]), 2, 2).permute(0, 2, 3, 1)
        assert torch.equal(out[s].double(), want), "max-pool forward %s, samples %s" % (name, s)


def check_pool_bwd(ch, name):
    """The upstream gradient routed to the first maximum of each window (float64 max_pool2d's saved argmax); with relu_mask the
    routed gradient times (x > 0), x the ReLU output the pool reads."""
    xin, _, _ = ch.fwd[name]
    _, g, dx, fuse, _, _ = ch.bwd[name]
    n = ch.n
    step = _chunk(n, xin[0].numel() * 2)
    for s0 in range(0, n, step):
        s = slice(s0, min(n, s0 + step))
        x64 = _nchw64(xin[s]).requires_grad_(True)
        (want,) = torch.autograd.grad(F.max_pool2d(x64, 2, 2), x64, _nchw64(g[s]))
        want = want.permute(0, 2, 3, 1)
        if fuse:
            want = want * (xin[s] > 0)
        assert torch.equal(dx[s].double(), want), "max-pool backward %s (relu_mask %d), samples %s" % (name, fuse, s)


def _entry_id(e):
    return "%s-N%d-%s-%s" % (e[4], e[3], e[0], e[1])


def _cases():
    return [e for e in TABLE] + [e for e in ODD_TABLE]


def _case_order(e):
    return (e[4] != "fp32", e[3] != NB)


@pytest.mark.parametrize("entry", sorted(_cases(), key=_case_order), ids=_entry_id)
def test_table_entry_vs_float64(hip, entry):
    """One (pass, op, kernel, N, math) of the tables: the chain's call of it showed that kernel, and its result is float64's on
    the chain's own operands."""
    pas, name, kernel, n, math = entry
    ch = _chain(hip, math, n)
    if pas == "fwd":
        _expect(ch.fwd[name][2], kernel, pas, name, n, math)
    elif pas == "act":
        _expect(ch.bwd[name][4], kernel, pas, name, n, math)
    else:
        _expect(ch.bwd[name][5], kernel, pas, name, n, math)
    if OP[name][1] == "pool":
        (check_pool_fwd if pas == "fwd" else check_pool_bwd)(ch, name)
        print("%s: bit-equal" % _entry_id(entry))
    elif pas == "act":
        check_act(ch, name)
        print("%s: bit-equal" % _entry_id(entry))
    elif pas == "fwd":
        err, tol = check_conv_fwd(ch, name), FWD_TOL[math]
        print("%s: forward %.3g (bound %.3g)" % (_entry_id(entry), err, tol))
        assert err <= tol, (entry, err)
    else:
        err, tol = check_conv_dgrad(ch, name), DGRAD_TOL[math]
        print("%s: data gradient %.3g (bound %.3g)" % (_entry_id(entry), err, tol))
        assert err <= tol, (entry, err)


# ------------------------------------------------------------------------------------------------------------ MSE and the term
CAP4 = 2048 * 256   # pws_sqdiff_sum's grid: at most 2048 workgroups of 256 float4 lanes, then a grid-stride loop
SQ_COUNTS4 = [1, 300, CAP4 - 1, CAP4, CAP4 + 1, 5 * CAP4 + 123]   # CAP4 = the features of 64 images (64 x 8 x 8 x 512 / 4)
SQ_SUM_TOL = 5e-7    # [sum 2.6e-8, mse 4.4e-8]  fp32 sums of <= 24 squares per lane, float64 after that; mse: its fp32 result
SQ_BWD_TOL = 2e-7    # [1.4e-7]  per element, relative to itself: (a - b), c * scale and the product rounded in fp32 (3 x 2^-24)


def _pair(count4, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(4 * count4, device="cuda", generator=g)
    b = a + 0.5 * torch.randn(4 * count4, device="cuda", generator=g)
    return a, b


@pytest.mark.parametrize("count4", SQ_COUNTS4)
def test_sqdiff_sum_and_mse_vs_float64(hip, count4):
    """pws_sqdiff_sum into the PWS_OBJ_SLOTS slots (their sum is sum (a - b)^2) and mse_loss's value (slots / count in
    pws_objective_finalize) against float64."""
    from pwstablenet_amd.perceptual import mse_loss
    A = hip
    L, st = A.lib(), A.current_stream()
    a, b = _pair(count4, 31 + count4)
    want = float(((a.double() - b.double()) ** 2).sum())
    slots = torch.zeros(A.OBJ_SLOTS, device="cuda", dtype=torch.float64)
    A.check(L.pws_sqdiff_sum(A.ptr(a), A.ptr(b), a.numel(), A.ptr(slots), st), "pws_sqdiff_sum")
    got = float(slots.sum())
    e_sum = abs(got - want) / want
    e_mse = abs(float(mse_loss(a, b)) - want / a.numel()) / (want / a.numel())
    print("count %d: sum %.3g, mse %.3g (bound %.3g)" % (a.numel(), e_sum, e_mse, SQ_SUM_TOL))
    assert e_sum <= SQ_SUM_TOL and e_mse <= SQ_SUM_TOL, (e_sum, e_mse)


@pytest.mark.parametrize("count4", SQ_COUNTS4)
def test_sqdiff_bwd_vs_float64(hip, count4):
    """ga = c * scale * 2 (a - b), with and without the device scale (the upstream gradient of the MSE), every element written."""
    A = hip
    L, st = A.lib(), A.current_stream()
    a, b = _pair(count4, 57 + count4)
    c = 1.0 / a.numel()
    scale = torch.tensor([0.75], device="cuda")
    worst = 0.0
    for sc in (None, scale):
        ga = torch.full_like(a, float("nan"))
        A.check(L.pws_sqdiff_bwd(A.ptr(a), A.ptr(b), a.numel(), c, A.ptr(sc) if sc is not None else None, A.ptr(ga), st),
                "pws_sqdiff_bwd")
        want = 2.0 * float(np.float32(c)) * (0.75 if sc is not None else 1.0) * (a.double() - b.double())   # c passes as fp32
        assert not torch.isnan(ga).any()
        worst = max(worst, float(((ga.double() - want).abs() / want.abs().clamp_min(1e-30)).max()))
    print("count %d: elementwise relative %.3g (bound %.3g)" % (a.numel(), worst, SQ_BWD_TOL))
    assert worst <= SQ_BWD_TOL, worst


# The gradient bounds are set by ReLU and argmax flips, not by rounding: a pre-activation within ~1e-6 of 0, or two values of a
# pool window within ~1e-6 of each other, go one way in fp32 and the other in float64, and each flip moves a receptive field of
# input gradient.  Against float64 the flips cost 3.5-5.8e-3 in relative L2 whatever the dither (1, 4 or 16 grey levels); the
# 64-image, 256 x 256 batch has far more of them than the 2-image, 64 x 64 one of test_hip_perceptual (5e-3 / 0.1 vs fp32 torch).
TERM_TOL = {"value": 1e-6,     # [8.5e-8]  rtol of the term (fp32 features: FWD_TOL per layer, the MSE in float64)
            "l2": 8e-3,        # [5.1e-3]  relative L2 of each fake's gradient
            "frac": 0.05,      # [0.024]  fraction of elements off by more than 2e-4 of max |gradient| (test_hip_perceptual: 0.1)
            "bf16": 1e-4}      # [3.6e-5]  rtol of the bf16 term against the store_bf16 oracle model


DITHER = 1.0   # grey levels (peak to peak) of the dither of the term's frames


def _dithered(n, seed, grey=DITHER):
    """synth frames plus a seeded dither of +-grey / 2 grey levels.  The plain frames are flat over about 11 % of their 2 x 2
    windows: there the float64 chain meets exact ties in the max-pool windows (equal im2col rows give equal sums), which the fp32
    Winograd tiles break one way or the other -- each a different argmax, i.e. a different valid subgradient.  On the plain frames
    the term's input gradients differ from float64 by 7-9 % in relative L2 for that reason alone (measured); the dither removes
    the exact ties."""
    x = _images(n, seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    return x + (torch.rand(x.shape, device="cuda", generator=g) - 0.5) * (grey / 127.5)


def _stages(grey=DITHER):
    return [_dithered(NB, 100 + k, grey) for k in range(3)], _dithered(NB, 200, grey)


def term_errors(fakes, stable):
    """(relative error of the fp32 term's value, [(relative L2, fraction of elements off by more than 2e-4 of max |gradient|) of
    the gradient wrt each fake]) against the float64 oracle chain."""
    from oracle import objective_ref
    from pwstablenet_amd.perceptual import GeneratorLoss, perceptual_term
    vgg = _vgg("fp32")
    fk = [f.clone().requires_grad_(True) for f in fakes]
    loss = perceptual_term(GeneratorLoss(vgg))(fk, stable)
    loss.backward()
    torch.cuda.synchronize()
    p64 = [t.detach().double() for m in vgg._convs() for t in (m.weight, m.bias)]
    step = 16
    with torch.backends.cudnn.flags(enabled=False):
        with torch.no_grad():
            ft = torch.cat([objective_ref.vgg16_features(p64, stable[s0:s0 + step].double()) for s0 in range(0, NB, step)])
        count = ft.numel()
        value, grads = 0.0, []
        for f in fakes:
            gr = torch.empty(f.shape, device="cuda", dtype=torch.float64)
            for s0 in range(0, NB, step):
                x64 = f[s0:s0 + step].double().requires_grad_(True)
                part = 2.0 * ((objective_ref.vgg16_features(p64, x64) - ft[s0:s0 + step]) ** 2).sum() / count
                (gr[s0:s0 + step],) = torch.autograd.grad(part, x64)
                value += float(part)
            grads.append(gr)
    rows = []
    for f, gr in zip(fk, grads):
        got = f.grad.double()
        l2 = float(torch.linalg.vector_norm(got - gr) / torch.linalg.vector_norm(gr))
        frac = float(((got - gr).abs() > 2e-4 * gr.abs().max()).double().mean())
        rows.append((l2, frac))
    return abs(float(loss) - value) / value, rows


def test_perceptual_term_vs_float64_oracle(hip):
    """perceptual_term(GeneratorLoss(VGG16Features('fp32'))) on 3 stages x 64 fakes + 64 stable frames against the float64
    oracle chain (oracle/objective_ref.py vgg16_features) on the device: the value, and the gradient wrt every fake (ReLU and
    argmax flips between fp32 and float64 move single elements: relative L2 plus a fraction-of-elements bound)."""
    ev, rows = term_errors(*_stages())
    print("fp32 perceptual term: value %.3g (bound %.3g); gradients (rel L2, fraction): %s" % (
        ev, TERM_TOL["value"], ", ".join("%.3g / %.3g" % r for r in rows)))
    assert ev <= TERM_TOL["value"], ev
    for l2, frac in rows:
        assert l2 <= TERM_TOL["l2"] and frac <= TERM_TOL["frac"], (l2, frac)


def test_perceptual_term_bf16_value_vs_the_bf16_oracle_model(hip):
    """bf16 math: the value of the term against the oracle's store_bf16 model (weights, input and every layer's output rounded to
    bf16, fp32 sums) on the device."""
    from oracle import objective_ref
    from pwstablenet_amd.perceptual import GeneratorLoss, perceptual_term
    vgg = _vgg("bf16")
    fakes, stable = _stages()
    with torch.no_grad():
        loss = float(perceptual_term(GeneratorLoss(vgg))(fakes, stable))
    p32 = [t.detach() for m in vgg._convs() for t in (m.weight, m.bias)]
    step = 16
    with torch.backends.cudnn.flags(enabled=False), torch.no_grad():
        feat = lambda x: torch.cat([objective_ref.vgg16_features(p32, x[s0:s0 + step], store_bf16=True)  # noqa: E731
                                    for s0 in range(0, NB, step)]).double()
        ft = feat(stable)
        value = sum(2.0 * float(((feat(f) - ft) ** 2).mean()) for f in fakes)
    ev = abs(loss - value) / value
    print("bf16 perceptual term: value %.3g (bound %.3g)" % (ev, TERM_TOL["bf16"]))
    assert ev <= TERM_TOL["bf16"], ev
