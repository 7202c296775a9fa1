"""The generator's conv layers at the batches of a training step (BASELINE configs[2] / [3]: 32 item pairs = 64 windows, ngf 64),
against float64.

1. The launch table.  One generator step at ngf 64 and n = 64 windows, bf16 and fp32 math, run under the profiler: every conv-family
   launch gives (pass, layer, kernel, N, pair).  N is the record's flops over the layer's flops per sample: n, 2n where stages 2
   and 3 run in lockstep (forward), or 2n for the backward's operand-pair weight-gradient launches (gout2 / src2_ptr).  TABLE below
   is that list, committed; test_live_launch_table_equals_the_committed_one recomputes it from a live step.  A dispatch change
   fails there until the table (and with it the cases of part 2) is updated.  The profiler names kernel families: the tile shapes
   inside one family (wgrad_bf16_kernel's 1-, 4- and 16-sample tiles) are not told apart by the table, but every one of them runs
   in part 2 at the N the step gives it.
2. Every entry of the table through the C ABI (pws_conv2d_fwd / _bwd_data / _bwd_weight) with the layer's real arguments: the
   source split of the virtual concat (ld = channels, as the executor's group buffers), the weight packs the executor hands that
   layer in that math (Winograd / ring copies in fp32, bf16 packs in bf16), the forward's act and sign bits, the data gradient's
   fused act' (with the forward tensor's sign bits where the executor keeps them) and accumulating destinations, dbias, and both
   operand pairs for the pair launches.  The profiler must show the kernel of the table.  Data are seeded random tensors made on
   the device, distinct per sample; bf16 operands are rounded once and the reference sees the rounded values.  The reference is
   torch in float64 on the device (with cudnn/MIOpen disabled: float64 convolutions run torch's own im2col + GEMM), over the
   WHOLE batch and every channel, in chunks of samples.  Deterministic mode and PWS_OPT_EXPERIMENT 190 (no tiles-per-workgroup
   floor) on the weight-gradient entries of the deep levels.
3. Batch additivity of the whole step: for a loss that is a sum over samples (use_BN off) the 92 gradients of one n = 64 step are
   the sum of those of eight n = 8 steps over the same windows, and the 64 per-sample fields are those of the n = 8 steps.  This
   covers the executor's arena offsets, the lockstep 2n tensors and the pair pointers at a training batch.

Bounds are relative to the tensor's largest float64 value, with the largest error measured on an MI355X in brackets.  The
per-layer bounds are those of tests/test_hip_sweep.py and tests/test_hip_bf16.py for the same operations, or tighter; the
additivity bounds are those of test_hip_backward's whole-generator check (why: above ADD_TOL).
"""
import ctypes
import zlib

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from pwstablenet_amd import spec, synth  # noqa: E402
from pwstablenet_amd.hipabi import Exp  # noqa: E402

pytestmark = pytest.mark.gpu

NGF, NB, S = 64, 64, 256            # the product's width, the step's batch (32 item pairs, two forwards as one), the window
SPECS = spec.layer_specs(31, 2, NGF)
HEADS = (15, 44, 45)                 # out (field head), flatten, linear (theta head): kernels of their own (tests/test_hip_heads.py)
WGRAD_KERNELS = ("wgrad_mfma_kernel", "wgrad_bf16_kernel", "wgrad_ring_kernel")
RING_LAYERS = {0, 11, 12, 13, 14, 16, 18, 20, 22, 36, 37, 38, 39, 40, 41, 42, 43}   # netg_layers.cpp build_layers(ring = true)

# bounds (relative to max |float64 reference| of the whole tensor).  fp32 math: exact-fp32 products; the error is the rounding of the
# fp32 sums (chains of cin * taps terms per output, in the orders of tiles, K splits and Winograd transforms), far below the
# worst-case chain bound (2^-24 per addition).  bf16 math: the operands are rounded before the call (exact products in fp32), so
# what is left is the bf16 rounding of a stored result (2^-9 of the value) and the fp32 summation order.
FWD_TOL = {"fp32": 2e-5,    # [3.0e-6]  (test_hip_sweep: 5e-5)
           "bf16": 6e-3}    # [3.5e-3]  one bf16 rounding of the result (test_hip_sweep TOL)
DGRAD_TOL = {"fp32": 2e-5,  # [3.3e-6]  the same kernels on dy (test_hip_sweep: 5e-5 / 2 * 6e-3)
             "bf16": 6e-3}  # [3.4e-3]  accumulated destinations and act' rounded once with the sum
WGRAD_TOL = {"fp32": 2e-5,  # [2.3e-6; deterministic 3.9e-6]  sums over N * H * W pixels in tiles, splits, atomics (test_hip_sweep 2e-4)
             "bf16": 2e-5}  # [1.9e-6; deterministic 6.6e-6]  summation order only; dbias [5.7e-7] (test_hip_bf16: 1e-4)


# ------------------------------------------------------------------------------------------------------------ layer geometry
def _kname(ls):
    if ls.kind == "conv":
        return {(5, 1): "CONV_K5S1", (3, 1): "CONV_K3S1", (3, 2): "CONV_K3S2"}[(ls.k, ls.s)]
    return {(3, 1): "CONVT_K3S1", (4, 2): "CONVT_K4S2"}[(ls.k, ls.s)]


def _layer(li):
    """(kname, input side, [source channels], [producer act of each source], cout, act of the output) of layer li as the executor
    runs it (netg_forward.cpp forward_lockstep: x_sk, conv_same outputs, d_s(l) = cat(v_sl, x_sl))."""
    g = NGF
    enc_c = [0, g, g, 2 * g, 4 * g, 4 * g, 4 * g, 4 * g, 4 * g]
    dec_c = [0, g, g, 2 * g, 4 * g, 4 * g, 4 * g, 4 * g]
    side = lambda k: S >> (k - 1)   # noqa: E731
    LR, RE = "ACT_LRELU", "ACT_RELU"
    ls = SPECS[li]
    kn = _kname(ls)

    def dec(l):   # d(l): channels and producer acts
        return ([enc_c[8]], [LR]) if l == 8 else ([dec_c[l], enc_c[l]], [RE, LR])
    if li == 0:
        h, src, acts, act = S, [31], [None], LR
    elif 1 <= li <= 7:                                  # down i on x_1i
        h, src, acts, act = side(li), [enc_c[li]], [LR], LR
    elif 8 <= li <= 14:                                 # up l on d_1(l + 1)
        lv = 7 - (li - 8)
        (src, acts), h, act = dec(lv + 1), side(lv + 1), RE
    elif 16 <= li <= 29:
        k = (li - 16) // 2 + 1
        h, act = side(k), LR
        if (li - 16) % 2 == 0:                          # down_bottom k conv_same on x_1k
            src, acts = [enc_c[k]], [LR]
        else:                                           # down_bottom k mpconv on cat(x_left, conv_same)
            src, acts = ([enc_c[k]], [LR]) if k == 1 else ([enc_c[k], enc_c[k]], [LR, LR])
    else:
        lv = 7 - (li - 30) // 2
        h, act = side(lv + 1), RE
        c_up, a_up = dec(lv + 1)
        if (li - 30) % 2 == 1:                          # up_bottom l conv_same on d(l + 1)
            src, acts = c_up, a_up
        else:                                           # up_bottom l mpconv on cat(conv_same output, d(l + 1) of the next stage)
            src, acts = [sum(c_up)] + c_up, [RE] + a_up
    assert sum(src) == ls.cin, (li, src, ls.cin)
    return kn, h, src, acts, ls.cout, act


def _geom(kn, h):
    """(k, stride, pad, transposed, output side, taps per output pixel in the flops count)"""
    return {"CONV_K5S1": (5, 1, 2, False, h, 25), "CONV_K3S1": (3, 1, 1, False, h, 9), "CONV_K3S2": (3, 2, 1, False, h // 2, 9),
            "CONVT_K3S1": (3, 1, 1, True, h, 9), "CONVT_K4S2": (4, 2, 1, True, 2 * h, 4)}[kn]


def _flops_per_sample(li, math):
    kn, h, src, _, cout, _ = _layer(li)
    cin = 32 if (li == 0 and math == "bf16") else sum(src)   # bf16: the window re-laid as 32 NHWC channels
    _, _, _, _, oh, k2 = _geom(kn, h)
    return 2.0 * oh * oh * cout * cin * k2


# ------------------------------------------------------------------------------------------------------------ the committed table
# (pass, layer, kernel, N, pair, math, store) of one ngf-64 step at n = 64 (recomputed by test_live_launch_table_equals_the_committed_one)
TABLE = [
    ('dgrad', 1, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 2, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 3, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 4, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 5, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 6, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 7, 'conv_skinny16_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 8, 'conv_skinny16_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 9, 'conv_bf16_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 10, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 11, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 12, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 13, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 14, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 16, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 17, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 18, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 19, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 20, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 21, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 22, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 23, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 24, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 25, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 26, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 27, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 28, 'conv_bf16_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 29, 'conv_skinny16_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 30, 'conv_skinny16_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 31, 'conv_skinny16_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 32, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 33, 'conv_bf16_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 34, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 35, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 36, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 37, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 38, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 39, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 40, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 41, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 42, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('dgrad', 43, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 0, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 1, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 2, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 3, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 4, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 5, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 6, 'conv_bf16_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 7, 'conv_skinny16_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 8, 'conv_skinny16_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 9, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 10, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 11, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 12, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 13, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 14, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 16, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 17, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 18, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 19, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 20, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 21, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 22, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 23, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 24, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 25, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 26, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 27, 'conv_bf16_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 28, 'conv_bf16_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 29, 'conv_bf16_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 30, 'conv_bf16_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 31, 'conv_bf16_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 32, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 33, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 34, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 35, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 36, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 37, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 38, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 39, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 40, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 41, 'conv_ring_kernel', 128, False, 'bf16', 'bf16'),
    ('fwd', 42, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('fwd', 43, 'conv_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 0, 'wgrad_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 1, 'wgrad_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 2, 'wgrad_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 3, 'wgrad_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 4, 'wgrad_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 5, 'wgrad_bf16_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 6, 'wgrad_bf16_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 7, 'wgrad_bf16_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 8, 'wgrad_bf16_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 9, 'wgrad_bf16_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 10, 'wgrad_bf16_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 11, 'wgrad_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 12, 'wgrad_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 13, 'wgrad_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 14, 'wgrad_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 16, 'wgrad_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 17, 'wgrad_ring_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 18, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 19, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 20, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 21, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 22, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 23, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 24, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 25, 'wgrad_bf16_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 26, 'wgrad_bf16_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 27, 'wgrad_bf16_kernel', 64, False, 'bf16', 'bf16'),
    ('wgrad', 28, 'wgrad_bf16_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 29, 'wgrad_bf16_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 30, 'wgrad_bf16_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 31, 'wgrad_bf16_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 32, 'wgrad_bf16_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 33, 'wgrad_bf16_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 34, 'wgrad_bf16_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 35, 'wgrad_bf16_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 36, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 37, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 38, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 39, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 40, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 41, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 42, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('wgrad', 43, 'wgrad_ring_kernel', 128, True, 'bf16', 'bf16'),
    ('dgrad', 1, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 2, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 3, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 4, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 5, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 6, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 7, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 8, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 9, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 10, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 11, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 12, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 13, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 14, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 16, 'conv_mfma_kernel<k3s1,16x16>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 17, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 18, 'conv_mfma_kernel<k3s1,16x16>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 19, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 20, 'conv_mfma_kernel<k3s1,16x16>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 21, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 22, 'conv_mfma_kernel<k3s1,16x16>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 23, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 24, 'conv_mfma_kernel<k3s1,16x16>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 25, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 26, 'conv_mfma_kernel<k3s1,small>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 27, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 28, 'conv_mfma_kernel<k3s1,small>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 29, 'conv_mfma_kernel<dgrad subpix k3s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 30, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 31, 'conv_mfma_kernel<k3s1,small>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 32, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 33, 'conv_mfma_kernel<k3s1,small>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 34, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 35, 'conv_mfma_kernel<k3s1,16x16>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 36, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 37, 'conv_mfma_kernel<k3s1,16x16>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 38, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 39, 'conv_mfma_kernel<k3s1,16x16>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 40, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 41, 'conv_mfma_kernel<k3s1,16x16>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 42, 'conv_mfma_kernel<dgrad k4s2>', 64, False, 'fp32', 'fp32'),
    ('dgrad', 43, 'conv_mfma_kernel<k3s1,16x16>', 64, False, 'fp32', 'fp32'),
    ('fwd', 0, 'wino5_first_kernel', 64, False, 'fp32', 'fp32'),
    ('fwd', 1, 'conv_ringf_kernel', 64, False, 'fp32', 'fp32'),
    ('fwd', 2, 'conv_ringf_kernel', 64, False, 'fp32', 'fp32'),
    ('fwd', 3, 'conv_ringf_kernel', 64, False, 'fp32', 'fp32'),
    ('fwd', 4, 'conv_mfma_kernel<k3s2,16x16>', 64, False, 'fp32', 'fp32'),
    ('fwd', 5, 'conv_mfma_kernel<k3s2,small>', 64, False, 'fp32', 'fp32'),
    ('fwd', 6, 'conv_mfma_kernel<k3s2,small>', 64, False, 'fp32', 'fp32'),
    ('fwd', 7, 'conv_mfma_kernel<k3s2,small>', 64, False, 'fp32', 'fp32'),
    ('fwd', 8, 'conv_mfma_kernel<convT4,small>', 64, False, 'fp32', 'fp32'),
    ('fwd', 9, 'conv_mfma_kernel<convT4,small>', 64, False, 'fp32', 'fp32'),
    ('fwd', 10, 'conv_mfma_kernel<convT4,16x16>', 64, False, 'fp32', 'fp32'),
    ('fwd', 11, 'wino_ring_kernel<convT4,F(2x2,2x2)>', 64, False, 'fp32', 'fp32'),
    ('fwd', 12, 'wino_ring_kernel<convT4,F(2x2,2x2)>', 64, False, 'fp32', 'fp32'),
    ('fwd', 13, 'wino_ring_kernel<convT4,F(2x2,2x2)>', 64, False, 'fp32', 'fp32'),
    ('fwd', 14, 'wino_ring_kernel<convT4,F(2x2,2x2)>', 64, False, 'fp32', 'fp32'),
    ('fwd', 16, 'wino_ring_kernel<F(2x2,3x3)>', 64, False, 'fp32', 'fp32'),
    ('fwd', 17, 'conv_ringf_kernel', 64, False, 'fp32', 'fp32'),
    ('fwd', 18, 'wino_ring_kernel<F(2x2,3x3)>', 128, False, 'fp32', 'fp32'),
    ('fwd', 19, 'conv_ringf_kernel', 64, False, 'fp32', 'fp32'),
    ('fwd', 20, 'wino_ring_kernel<F(2x2,3x3)>', 128, False, 'fp32', 'fp32'),
    ('fwd', 21, 'conv_ringf_kernel', 128, False, 'fp32', 'fp32'),
    ('fwd', 22, 'wino_ring_kernel<F(2x2,3x3)>', 128, False, 'fp32', 'fp32'),
    ('fwd', 23, 'conv_mfma_kernel<k3s2,16x16>', 128, False, 'fp32', 'fp32'),
    ('fwd', 24, 'wino_k3s1_kernel<F(2x2,3x3)>', 128, False, 'fp32', 'fp32'),
    ('fwd', 25, 'conv_mfma_kernel<k3s2,16x16>', 128, False, 'fp32', 'fp32'),
    ('fwd', 26, 'conv_mfma_kernel<k3s1,16x16>', 128, False, 'fp32', 'fp32'),
    ('fwd', 27, 'conv_mfma_kernel<k3s2,small>', 128, False, 'fp32', 'fp32'),
    ('fwd', 28, 'conv_mfma_kernel<k3s1,small>', 128, False, 'fp32', 'fp32'),
    ('fwd', 29, 'conv_mfma_kernel<k3s2,small>', 128, False, 'fp32', 'fp32'),
    ('fwd', 30, 'conv_mfma_kernel<convT4,small>', 128, False, 'fp32', 'fp32'),
    ('fwd', 31, 'conv_mfma_kernel<k3s1,small>', 128, False, 'fp32', 'fp32'),
    ('fwd', 32, 'conv_mfma_kernel<convT4,small>', 128, False, 'fp32', 'fp32'),
    ('fwd', 33, 'conv_mfma_kernel<k3s1,small>', 128, False, 'fp32', 'fp32'),
    ('fwd', 34, 'conv_mfma_kernel<convT4,16x16>', 128, False, 'fp32', 'fp32'),
    ('fwd', 35, 'conv_mfma_kernel<k3s1,16x16>', 128, False, 'fp32', 'fp32'),
    ('fwd', 36, 'wino_ring_kernel<convT4,F(2x2,2x2)>', 128, False, 'fp32', 'fp32'),
    ('fwd', 37, 'wino_ring_kernel<F(2x2,3x3)>', 128, False, 'fp32', 'fp32'),
    ('fwd', 38, 'wino_ring_kernel<convT4,F(2x2,2x2)>', 128, False, 'fp32', 'fp32'),
    ('fwd', 39, 'wino_ring_kernel<F(2x2,3x3)>', 128, False, 'fp32', 'fp32'),
    ('fwd', 40, 'wino_ring_kernel<convT4,F(2x2,2x2)>', 128, False, 'fp32', 'fp32'),
    ('fwd', 41, 'wino_ring_kernel<F(2x2,3x3)>', 128, False, 'fp32', 'fp32'),
    ('fwd', 42, 'wino_ring_kernel<convT4,F(2x2,2x2)>', 64, False, 'fp32', 'fp32'),
    ('fwd', 43, 'wino_ring_kernel<F(2x2,3x3)>', 64, False, 'fp32', 'fp32'),
    ('wgrad', 0, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 1, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 2, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 3, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 4, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 5, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 6, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 7, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 8, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 9, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 10, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 11, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 12, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 13, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 14, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 16, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 17, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 18, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 19, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 20, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 21, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 22, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 23, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 24, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 25, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 26, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 27, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 28, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 29, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 30, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 31, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 32, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 33, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 34, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 35, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 36, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 37, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 38, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 39, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 40, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 41, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 42, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
    ('wgrad', 43, 'wgrad_mfma_kernel', 64, False, 'fp32', 'fp32'),
]


def _make_net(math):
    from pwstablenet_amd.lib.networks_cascading import define_G
    net = define_G(31, 2, NGF, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=NGF)})
    net = net.cuda()
    net.module.set_math(math)
    return net


def _step_inputs(n, seed=2027):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((n, 31, S, S), device="cuda", generator=g) * 2 - 1
    tf = torch.randn((n, S, S, 2), device="cuda", generator=g) * 0.3
    return x, tf


def _sum_loss(grids, resid, tf):
    """A sum over samples (and pixels): the gradients of a batch are the sums of those of its parts."""
    return sum(((g_ - tf) ** 2).sum() for g_ in grids) + 0.1 * sum((r * r).sum() for r in resid)


def live_table(hip, math):
    """The launch table of one step (sorted, duplicates removed)."""
    A = hip
    L = A.lib()
    net = _make_net(math)
    x, tf = _step_inputs(NB)
    net.zero_grad()
    store = net.module.store
    L.pws_prof_enable(1)
    try:
        grids, resid = net(x)
        torch.cuda.synchronize()
        fwd = A.prof_collect()
        _sum_loss(grids, resid, tf).backward()
        torch.cuda.synchronize()
        bwd = A.prof_collect()
    finally:
        L.pws_prof_enable(0)
    out = set()
    for pas, recs in (("fwd", fwd), ("bwd", bwd)):
        for name, tag, flops, _, _ in recs:
            if tag < 0 or tag in HEADS:
                continue
            if name in WGRAD_KERNELS:
                p = "wgrad"
            elif name.startswith(("conv_", "wino")):
                p = "fwd" if pas == "fwd" else "dgrad"
            else:
                continue   # act' / bias sums, layout copies, the heads
            per = _flops_per_sample(tag, math)
            nn_ = int(round(flops / per))
            assert nn_ * per == flops and nn_ in (NB, 2 * NB), (name, tag, flops, per)
            out.add((p, tag, name, nn_, p == "wgrad" and nn_ == 2 * NB, math, store))
    return sorted(out)


@pytest.mark.parametrize("math", ["bf16", "fp32"])
def test_live_launch_table_equals_the_committed_one(hip, math):
    """The tripwire: a dispatch change (kernel, N, pair) at the training batch fails here until TABLE and the cases follow it."""
    live = live_table(hip, math)
    want = sorted(e for e in TABLE if e[5] == math)
    missing, extra = sorted(set(want) - set(live)), sorted(set(live) - set(want))
    assert not missing and not extra, "launch table changed:\n  gone: %s\n  new:  %s" % (missing, extra)
    # every layer of the step has its three passes (the first layer: no data gradient) in the table
    for li in range(len(SPECS)):
        if li in HEADS:
            continue
        passes = {e[0] for e in live if e[1] == li}
        assert passes == ({"fwd", "wgrad"} if li == 0 else {"fwd", "dgrad", "wgrad"}), (li, passes)


# ------------------------------------------------------------------------------------------------------------ per-entry checks
def _rand(shape, gen, dtype):
    t = torch.randn(shape, device="cuda", generator=gen)
    return t.to(dtype)


def _sign_bits(y):
    """pws_conv_args.out_sign layout of a [.., c] bf16 tensor: bit (c & 7) of byte [pixel][c / 8] = (y > 0)."""
    c = y.shape[-1]
    b = (y.float() > 0).reshape(-1, c // 8, 8).to(torch.int32)
    return (b << torch.arange(8, device=y.device, dtype=torch.int32)).sum(-1).to(torch.uint8)


def _chunk(n, per_sample_elems):
    return max(1, min(n, int((1 << 27) // max(per_sample_elems, 1))))   # ~1 GB of float64 per operand


class _Layer:
    """Weights and every pack the executor hands layer li in `math`."""

    def __init__(self, A, li, math):
        L, st = A.lib(), A.current_stream()
        self.li, self.math = li, math
        self.kn, self.h, self.src, self.acts, self.cout, self.act = _layer(li)
        self.kind = getattr(A, self.kn)
        self.k, self.s, self.p, self.tr, self.oh, _ = _geom(self.kn, self.h)
        self.cin = sum(self.src)
        g = torch.Generator().manual_seed(zlib.crc32(repr(("w", li)).encode()))
        shp = spec.weight_shape(SPECS[li])
        self.wt = (torch.randn(shp, generator=g) / (self.cin * self.k * self.k) ** 0.5).cuda()
        self.b = torch.randn(self.cout, generator=g).cuda() * 0.1
        self.w64 = (self.wt.bfloat16() if math == "bf16" else self.wt).double()   # the bf16 packs round once (RNE)
        kind, cin, cout = self.kind, self.cin, self.cout
        self.wp = torch.empty(L.pws_packed_weight_floats(kind, cin, cout), device="cuda")
        A.check(L.pws_pack_conv_weight(A.ptr(self.wt), A.ptr(self.wp), kind, cin, cout, st), "pack")
        self.wb = self.wino = self.wring = None
        if math == "bf16":
            planes = {"CONV_K5S1": 25, "CONVT_K4S2": 16}.get(self.kn, 9)
            cpad = (cin + 15) // 16 * 16
            self.wb = torch.empty(L.pws_packed_bf16_floats(planes, cpad, cout), device="cuda")
            A.check(L.pws_pack_weight_bf16(A.ptr(self.wp), A.ptr(self.wb), planes, cpad, cout, st), "pack_bf16")
        else:
            if self.kn in ("CONV_K3S1", "CONVT_K3S1"):
                self.wino = torch.empty(L.pws_packed_wino_floats(cin, cout), device="cuda")
                A.check(L.pws_pack_conv_weight_wino(A.ptr(self.wp), A.ptr(self.wino), cin, cout, st), "pack_wino")
            nr = L.pws_packed_wring_floats(kind, cin, cout)
            if li in RING_LAYERS and nr:
                self.wring = torch.empty(nr, device="cuda")
                A.check(L.pws_pack_conv_weight_wring(A.ptr(self.wp), A.ptr(self.wring), kind, cin, cout, st), "pack_wring")
        if li != 0:
            self.wdg = torch.empty(L.pws_packed_dgrad_floats(kind, cin, cout), device="cuda")
            A.check(L.pws_pack_conv_weight_dgrad(A.ptr(self.wt), A.ptr(self.wdg), kind, cin, cout, st), "pack_dgrad")
            self.wdb = None
            if math == "bf16":
                dplanes = 9 if "S1" in self.kn else 16
                self.wdb = torch.empty(L.pws_packed_bf16_floats(dplanes, cout, cin), device="cuda")
                A.check(L.pws_pack_weight_bf16(A.ptr(self.wdg), A.ptr(self.wdb), dplanes, cout, cin, st), "pack_bf16 dgrad")

    def conv64(self, x, w=None, bias=None):
        """float64 NCHW forward of the layer (torch's own kernels: cudnn is off around every call)."""
        w = self.w64 if w is None else w
        if self.tr:
            return F.conv_transpose2d(x, w, bias, stride=self.s, padding=self.p)
        return F.conv2d(x, w, bias, stride=self.s, padding=self.p)


def _act64(z, act):
    return torch.where(z > 0, z, z * (0.2 if act == "ACT_LRELU" else 0.0))


def _dact(y, act):
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.2 if act == "ACT_LRELU" else 0.0))


class _Err:
    def __init__(self):
        self.num, self.den = 0.0, 0.0

    def add(self, got, want):
        self.num = max(self.num, float((got.double() - want).abs().max()))
        self.den = max(self.den, float(want.abs().max()))

    @property
    def rel(self):
        return self.num / max(self.den, 1e-30)


def _profiled(A, fn):
    L = A.lib()
    L.pws_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.pws_prof_enable(0)
    return A.prof_collect()


def _expect(recs, kernel, li, n, math):
    names = [r[0] for r in recs]
    assert names == [kernel], (names, kernel)
    per = _flops_per_sample(li, math)
    assert recs[0][2] == per * n, (recs[0][2], per * n)


def _ws():
    return torch.empty(256 << 20, dtype=torch.uint8, device="cuda")


def check_fwd(A, ly, n, kernel, seed):
    L, st = A.lib(), A.current_stream()
    math = ly.math
    bf = math == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    gen = torch.Generator(device="cuda").manual_seed(seed)
    h, oh = ly.h, ly.oh
    a = A.PwsConvArgs()
    a.kind, a.n, a.h, a.w, a.cout, a.act = ly.kind, n, h, h, ly.cout, getattr(A, ly.act)
    if ly.li == 0 and not bf:                      # the NCHW window
        x = _rand((n, 31, h, h), gen, torch.float32)
        a.nsrc, a.src_nchw = 1, 1
        a.src[0].ptr, a.src[0].channels, a.src[0].ld = x.data_ptr(), 31, 0
        srcs = [x]
        x64 = lambda s: x[s].double()               # noqa: E731
    else:
        chans = [32] if ly.li == 0 else ly.src
        srcs = [_rand((n, h, h, c), gen, dt) for c in chans]
        if ly.li == 0:
            srcs[0][..., 31] = 0                    # the 32nd channel of the re-laid window is padding
        a.nsrc = len(srcs)
        for i, (t, c) in enumerate(zip(srcs, chans)):
            a.src[i].ptr, a.src[i].channels, a.src[i].ld = t.data_ptr(), c, c
        x64 = lambda s: torch.cat([t[s] for t in srcs], -1)[..., :ly.cin].permute(0, 3, 1, 2).double()   # noqa: E731
    out = torch.full((n, oh, oh, ly.cout), float("nan"), device="cuda", dtype=dt)
    sign = None
    ws = _ws()
    a.w_packed, a.bias, a.out, a.out_ld = ly.wp.data_ptr(), ly.b.data_ptr(), out.data_ptr(), ly.cout
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    a.math, a.store = (A.MATH_BF16, A.STORE_BF16) if bf else (A.MATH_FP32, A.STORE_FP32)
    if bf:
        a.w_bf16 = ly.wb.data_ptr()
        if oh >= 32:                                # netg_exec.h wants_sign: the executor keeps the sign bits of this output
            sign = torch.zeros((n * oh * oh, ly.cout // 8), device="cuda", dtype=torch.uint8)
            a.out_sign, a.out_sign_ld = sign.data_ptr(), ly.cout // 8
    else:
        a.w_wino = ly.wino.data_ptr() if ly.wino is not None else None
        a.w_wring = ly.wring.data_ptr() if ly.wring is not None else None
    recs = _profiled(A, lambda: A.check(L.pws_conv2d_fwd(ctypes.byref(a), st), "fwd"))
    _expect(recs, kernel, ly.li, n, math)
    err = _Err()
    b64 = ly.b.double()
    step = _chunk(n, max(ly.cin * h * h, ly.cout * oh * oh) * 2)
    with torch.backends.cudnn.flags(enabled=False):
        for s0 in range(0, n, step):
            s = slice(s0, min(n, s0 + step))
            want = _act64(ly.conv64(x64(s), bias=b64), ly.act).permute(0, 2, 3, 1)
            err.add(out[s], want)
    assert not torch.isnan(out).any()
    if sign is not None:
        assert torch.equal(sign, _sign_bits(out.reshape(-1, ly.cout))), "out_sign"
    return err.rel


def check_dgrad(A, ly, n, kernel, seed):
    L, st = A.lib(), A.current_stream()
    math = ly.math
    bf = math == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    gen = torch.Generator(device="cuda").manual_seed(seed)
    h, oh = ly.h, ly.oh
    gout = _rand((n, oh, oh, ly.cout), gen, dt)
    da = A.PwsConvBwdDataArgs()
    da.kind, da.n, da.h, da.w, da.cout = ly.kind, n, h, h, ly.cout
    da.gout, da.gout_ld, da.w_dgrad, da.ndst = gout.data_ptr(), ly.cout, ly.wdg.data_ptr(), len(ly.src)
    da.math, da.store = (A.MATH_BF16, A.STORE_BF16) if bf else (A.MATH_FP32, A.STORE_FP32)
    if bf:
        da.w_dgrad_bf16 = ly.wdb.data_ptr()
    dsts, prev, ys, signs = [], [], [], []
    for i, c in enumerate(ly.src):
        acc = (i + ly.li) % 2          # both kinds of destination on every layer with two or more of them
        p_ = _rand((n, h, h, c), gen, dt) if acc else None
        o = p_.clone() if acc else torch.full((n, h, h, c), float("nan"), device="cuda", dtype=dt)
        dsts.append(o), prev.append(p_)
        da.dst[i].ptr, da.dst[i].channels, da.dst[i].ld, da.dst[i].accumulate = o.data_ptr(), c, c, acc
        y = sg = None
        if bf:                         # bf16: the executor fuses act' of the producer into the data gradient
            y = _rand((n, h, h, c), gen, dt)
            da.dst[i].act_y, da.dst[i].act_y_ld, da.dst[i].act = y.data_ptr(), c, getattr(A, ly.acts[i])
            if h >= 32:
                sg = _sign_bits(y.reshape(-1, c))
                da.dst[i].act_sign, da.dst[i].act_sign_ld = sg.data_ptr(), c // 8
        ys.append(y), signs.append(sg)
    ws = _ws()
    da.ws, da.ws_bytes = ws.data_ptr(), ws.numel()
    recs = _profiled(A, lambda: A.check(L.pws_conv2d_bwd_data(ctypes.byref(da), st), "dgrad"))
    _expect(recs, kernel, ly.li, n, math)
    errs = [_Err() for _ in ly.src]
    step = _chunk(n, max(ly.cin * h * h, ly.cout * oh * oh) * 3)
    with torch.backends.cudnn.flags(enabled=False):
        for s0 in range(0, n, step):
            s = slice(s0, min(n, s0 + step))
            x64 = torch.zeros((s.stop - s.start, ly.cin, h, h), device="cuda", dtype=torch.float64, requires_grad=True)
            y64 = ly.conv64(x64)
            (gx,) = torch.autograd.grad(y64, x64, gout[s].permute(0, 3, 1, 2).double())
            gx = gx.permute(0, 2, 3, 1)
            c0 = 0
            for i, c in enumerate(ly.src):
                want = gx[..., c0:c0 + c]
                if prev[i] is not None:
                    want = want + prev[i][s].double()
                if ys[i] is not None:
                    want = want * _dact(ys[i][s].double(), ly.acts[i])
                errs[i].add(dsts[i][s], want)
                c0 += c
    for o in dsts:
        assert not torch.isnan(o).any()
    return max(e.rel for e in errs)


def _shared(li):
    """Stages 2 and 3 both run the layer (down_bottom2..7, up_bottom7..1): the executor hands its weight gradient both operand pairs."""
    return 18 <= li <= 43


def check_wgrad(A, ly, n, kernel, pair, seed, deterministic=False, repeat=1):
    """The weight gradient as the step asks for it: a merged operand-pair launch of N = 2 n1 (pair), both operand pairs of a shared
    layer given to one call that runs them as two launches of n1 = N each, or one operand pair.  dbias taken along where the step
    does (bf16: the act' is fused upstream; fp32 sums the bias in a pass of its own).  Returns (error of dW, error of dbias or 0,
    [(dW, dbias) of every repeat])."""
    L, st = A.lib(), A.current_stream()
    math = ly.math
    bf = math == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    gen = torch.Generator(device="cuda").manual_seed(seed)
    h, oh = ly.h, ly.oh
    n1 = n // 2 if pair else n
    npairs = 2 if (pair or _shared(ly.li)) else 1
    nchw = ly.li == 0 and not bf
    chans = [32] if ly.li == 0 and bf else ly.src
    ops = []
    for _ in range(npairs):
        if nchw:
            srcs = [_rand((n1, 31, h, h), gen, torch.float32)]
        else:
            srcs = [_rand((n1, h, h, c), gen, dt) for c in chans]
            if ly.li == 0:
                srcs[0][..., 31] = 0
        ops.append((srcs, _rand((n1, oh, oh, ly.cout), gen, dt)))
    wa = A.PwsConvBwdWeightArgs()
    wa.kind, wa.n, wa.h, wa.w, wa.nsrc, wa.src_nchw = ly.kind, n1, h, h, len(chans), 1 if nchw else 0
    for i, (t, c) in enumerate(zip(ops[0][0], [31] if nchw else chans)):
        wa.src[i].ptr, wa.src[i].channels, wa.src[i].ld = t.data_ptr(), c, 0 if nchw else c
    wa.cout, wa.gout, wa.gout_ld = ly.cout, ops[0][1].data_ptr(), ly.cout
    if npairs == 2:
        for i, t in enumerate(ops[1][0]):
            wa.src2_ptr[i] = t.data_ptr()
        wa.gout2 = ops[1][1].data_ptr()
    wa.math, wa.store = (A.MATH_BF16, A.STORE_BF16) if bf else (A.MATH_FP32, A.STORE_FP32)
    wa.deterministic = 1 if deterministic else 0
    dws = []
    for _ in range(repeat):
        dwp = torch.zeros(L.pws_packed_weight_floats(ly.kind, ly.cin, ly.cout), device="cuda")
        db = torch.full((ly.cout,), 0.25, device="cuda")   # accumulated onto
        # (deterministic: the step sums the bias in an ordered pass of its own, and the kernels refuse dbias)
        wa.dw_packed, wa.dbias = dwp.data_ptr(), db.data_ptr() if (bf and not deterministic) else None
        recs = _profiled(A, lambda: A.check(L.pws_conv2d_bwd_weight(ctypes.byref(wa), st), "wgrad"))
        if npairs == 2 and not pair:   # the pair as two launches, one per operand pair
            assert [r[0] for r in recs] == [kernel, kernel], ([r[0] for r in recs], kernel)
            _expect(recs[:1], kernel, ly.li, n, math)
            _expect(recs[1:], kernel, ly.li, n, math)
        else:
            _expect(recs, kernel, ly.li, n, math)
        dw = torch.empty(tuple(ly.wt.shape), device="cuda")
        A.check(L.pws_unpack_conv_weight(A.ptr(dwp), A.ptr(dw), ly.kind, ly.cin, ly.cout, st), "unpack")
        torch.cuda.synchronize()
        dws.append((dw, db - 0.25))
    want_w = torch.zeros(tuple(ly.wt.shape), device="cuda", dtype=torch.float64)
    want_b = torch.zeros(ly.cout, device="cuda", dtype=torch.float64)
    step = _chunk(n1, max(ly.cin * h * h, ly.cout * oh * oh) * 2)
    with torch.backends.cudnn.flags(enabled=False):
        for srcs, gout in ops:
            for s0 in range(0, n1, step):
                s = slice(s0, min(n1, s0 + step))
                if nchw:
                    x64 = srcs[0][s].double()
                else:
                    x64 = torch.cat([t[s] for t in srcs], -1)[..., :ly.cin].permute(0, 3, 1, 2).double()
                w64 = ly.w64.clone().requires_grad_(True)
                g64 = gout[s].permute(0, 3, 1, 2).double()
                (gw,) = torch.autograd.grad(ly.conv64(x64, w64), w64, g64)
                want_w += gw
                want_b += g64.sum(dim=(0, 2, 3))
    ew, eb = _Err(), _Err()
    ew.add(dws[0][0], want_w)
    if bf and not deterministic:
        eb.add(dws[0][1], want_b)
    else:
        assert float(dws[0][1].abs().max()) == 0.0   # no dbias given: untouched
    return ew.rel, eb.rel, dws


def _entry_id(e):
    return "%s-%s-L%d-%s-N%d%s" % (e[5], e[0], e[1], SPECS[e[1]].name.split(".")[0], e[3], "-pair" if e[4] else "")


_layers = {}


def _get_layer(A, li, math):
    key = (li, math)
    if key not in _layers:
        _layers.clear()   # one layer's packs at a time (the cases are grouped by layer below)
        _layers[key] = _Layer(A, li, math)
    return _layers[key]


def _sorted_table():
    return sorted(TABLE, key=lambda e: (e[5], e[1], e[0], e[3]))


@pytest.mark.parametrize("entry", _sorted_table(), ids=_entry_id)
def test_table_entry_vs_float64(hip, entry):
    """One (pass, layer, kernel, N, pair, math, store) of the table through the C ABI against float64."""
    pas, li, kernel, n, pair, math, store = entry
    assert store == ("bf16" if math == "bf16" else "fp32")
    ly = _get_layer(hip, li, math)
    seed = zlib.crc32(repr(entry).encode())
    if pas == "fwd":
        err = check_fwd(hip, ly, n, kernel, seed)
        tol = FWD_TOL[math]
        print("%s: forward %.3g (bound %.3g)" % (_entry_id(entry), err, tol))
        assert err <= tol, (entry, err)
    elif pas == "dgrad":
        err = check_dgrad(hip, ly, n, kernel, seed)
        tol = DGRAD_TOL[math]
        print("%s: data gradient %.3g (bound %.3g)" % (_entry_id(entry), err, tol))
        assert err <= tol, (entry, err)
    else:
        ew, eb, _ = check_wgrad(hip, ly, n, kernel, pair, seed)
        tol = WGRAD_TOL[math]
        print("%s: weight gradient %.3g, dbias %.3g (bound %.3g)" % (_entry_id(entry), ew, eb, tol))
        assert ew <= tol and eb <= tol, (entry, ew, eb)


def _deep_wgrad():
    return [e for e in _sorted_table() if e[0] == "wgrad" and _layer(e[1])[1] <= 32]


@pytest.mark.parametrize("entry", _deep_wgrad(), ids=_entry_id)
def test_deep_weight_gradient_deterministic_and_without_tile_floor(hip, entry):
    """The weight-gradient entries of the deep levels (<= 32 x 32 inputs, where the pixel splits are few tiles each):
    deterministic mode (one adding workgroup per address: ps = 1) is bit-identical run to run and within the bound of float64;
    PWS_OPT_EXPERIMENT 190 (no tiles-per-workgroup floor: the other side of the round-6 floor of 6) is within the same bound."""
    A = hip
    pas, li, kernel, n, pair, math, store = entry
    ly = _get_layer(A, li, math)
    seed = zlib.crc32(repr(entry).encode())
    tol = WGRAD_TOL[math]
    ew, eb, dws = check_wgrad(A, ly, n, kernel, pair, seed, deterministic=True, repeat=2)
    assert torch.equal(dws[0][0], dws[1][0]) and torch.equal(dws[0][1], dws[1][1]), "deterministic runs differ"
    assert ew <= tol and eb <= tol, ("deterministic", entry, ew, eb)
    with A.experiment(Exp.WGRAD_MIN_TILES):
        ew2, eb2, _ = check_wgrad(A, ly, n, kernel, pair, seed)
    print("%s: deterministic %.3g / %.3g, no floor %.3g / %.3g (bound %.3g)" % (_entry_id(entry), ew, eb, ew2, eb2, tol))
    assert ew2 <= tol and eb2 <= tol, ("experiment 190", entry, ew2, eb2)


# ------------------------------------------------------------------------------------------------------------ batch additivity
# The bound of a gradient is set by activation branches, not by rounding: a pre-activation within rounding of 0 takes the other
# LeakyReLU / ReLU branch in one of the two computations (other kernels at n = 8 and n = 64 round it differently), and the
# element's gradient changes by a factor.  On the small deep maps one such element moves a whole tensor: the float64 step over
# the same windows is 2.4e-3 away from the n = 64 step on down6 and 8.9e-8 from the n = 8 steps, and the reverse on
# down_bottom6.  Run to run (atomics' order) the n = 64 step moves by <= 8e-7 (fp32).  The bounds are the caps of
# test_hip_backward's whole-generator check against float64 (_GRAD_TOL field / W1: 3e-3; W2, where branches flip: 3e-2).
ADD_TOL = {"fp32": (3e-3, 5e-6),   # (gradients, fields)  [gradients 2.35e-3 (down6.mpconv.0.weight); fields 5.0e-7]
           "bf16": (3e-2, 8e-3)}   # bf16 activations: roundings of stored values flip too  [gradients 1.9e-2; fields 3.5e-3]


@pytest.mark.parametrize("math", ["fp32", "bf16"])
def test_batch_additivity_of_the_step(hip, math):
    """One n = 64 step (distinct windows) against eight n = 8 steps over the same windows: every one of the 92 gradients is the
    sum of the parts' (the loss is a sum over samples, use_BN off), and every sample's six fields are the parts' fields."""
    net = _make_net(math)
    x, tf = _step_inputs(NB, seed=4242)

    def step(xs, ts):
        net.zero_grad()
        grids, resid = net(xs)
        _sum_loss(grids, resid, ts).backward()
        torch.cuda.synchronize()
        return [p.grad.double() for p in net.module._ordered_params()], [t.detach().double() for t in list(grids) + list(resid)]
    g_all, f_all = step(x, tf)
    g_sum = [torch.zeros_like(t) for t in g_all]
    f_parts = [[] for _ in f_all]
    for k in range(NB // 8):
        s = slice(8 * k, 8 * k + 8)
        g, f = step(x[s], tf[s])
        for a, b in zip(g_sum, g):
            a += b
        for lst, t in zip(f_parts, f):
            lst.append(t)
    rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)   # noqa: E731
    gtol, ftol = ADD_TOL[math]
    rows, bad = [], []
    for (name, _), a, b in zip(spec.param_specs(31, 2, NGF), g_all, g_sum):
        e = rel(b, a)
        rows.append((e, name))
        if e > gtol:
            bad.append("%s: %.3g" % (name, e))
    worst_f = 0.0
    for i, (a, parts) in enumerate(zip(f_all, f_parts)):
        e = rel(torch.cat(parts), a)
        worst_f = max(worst_f, e)
        if e > ftol:
            bad.append("field %d: %.3g" % (i, e))
    rows.sort(reverse=True)
    print("%s additivity: worst gradients %s (bound %.3g); worst field %.3g (bound %.3g)" % (
        math, "; ".join("%s %.2g" % (nm, e) for e, nm in rows[:5]), gtol, worst_f, ftol))
    assert not bad, "\n".join(bad)
