"""Single conv calls that reach each kernel family of the dispatch ladder (csrc/conv_dispatch.hip), shared by tests/test_conv_plan_cpu.py
(planned on fake addresses, no GPU) and tests/test_hip_conv_plan.py (planned and launched).  Each is the smallest row of an existing
GPU test that covers the family: the ring and Winograd-ring families only take a launch that fills the chip, so the small rows force
them with the experiment switch their own tests use.  Buffers are sized, never filled: these tests ask which kernel runs, not what it
computes."""
from pwstablenet_amd.hipabi import Exp

PLANES = {"CONV_K3S1": 9, "CONV_K3S2": 9, "CONVT_K3S1": 9, "CONVT_K4S2": 16, "CONV_K5S1": 25}
# (id, kind, (n, h, w) of the input, source channels, cout, mode, experiment, extra weights, kernel expected)
#   mode: fp32 | bf16 (bf16 math and storage) | nchw (the first layer's fp32 NCHW window, src_c[0] channels)
FWD_CASES = [
    ("ring", "CONV_K3S1", (1, 16, 32), [32], 64, "bf16", Exp.RING_UNIT256, (), "conv_ring_kernel"),              # test_hip_ring.py FWD_SMALL
    ("skinny16", "CONV_K3S1", (2, 4, 4), [32], 64, "bf16", 0, (), "conv_skinny16_kernel"),                       # test_hip_sweep.py: maps <= 8 x 8
    ("bf16", "CONV_K3S2", (2, 20, 32), [32], 64, "bf16", 0, (), "conv_bf16_kernel"),                             # test_hip_sweep.py: ragged tiles
    ("bf16_k5", "CONV_K5S1", (1, 24, 32), [32], 64, "bf16", Exp.RING_OFF, (), "conv_bf16_kernel"),               # test_hip_ring.py FWD, ring off
    ("wring", "CONVT_K3S1", (3, 16, 32), [64], 32, "fp32", Exp.WRING_FORCE, ("wring",), "wino_ring_kernel<F(2x2,3x3)>"),          # test_hip_ops.py, Winograd ring rows
    ("wring_ct4", "CONVT_K4S2", (2, 16, 32), [64], 32, "fp32", Exp.WRING_FORCE, ("wring",), "wino_ring_kernel<convT4,F(2x2,2x2)>"),
    ("wino", "CONV_K3S1", (4, 128, 128), [64, 64], 64, "fp32", 0, ("wino",), "wino_k3s1_kernel<F(2x2,3x3)>"),   # test_hip_ops.py, Winograd rows
    ("wino_ct4", "CONVT_K4S2", (4, 64, 64), [128, 64], 64, "fp32", 0, ("wino",), "wino_ct4_kernel<F(3x3,2x2)>"),
    ("ringf", "CONV_K3S1", (2, 16, 32), [16], 64, "fp32", Exp.RINGF_8X32, (), "conv_ringf_kernel"),              # test_hip_ops.py RINGF_CASES
    ("skinny", "CONV_K3S1", (5, 4, 4), [32], 32, "fp32", 0, (), "conv_skinny_kernel"),                           # test_hip_ops.py CONV_CASES
    ("mfma", "CONV_K3S1", (2, 20, 37), [16], 64, "fp32", 0, (), "conv_mfma_kernel<k3s1,small>"),                 # test_hip_ops.py CONV_CASES
    ("first", "CONV_K5S1", (2, 16, 32), [31], 64, "nchw", Exp.FIRST_SMALL, (), "conv_first_kernel"),             # test_hip_ops.py FIRST_CASES
    ("first_wino", "CONV_K5S1", (1, 8, 16), [31], 64, "nchw", Exp.WINO5_SMALL, ("wring",), "wino5_first_kernel"),   # test_hip_ops.py WINO5_CASES
]
# (id, kind, (n, h, w) of the forward input = extent of dx, forward sources = destinations, forward cout, mode, experiment, kernel expected)
BWD_CASES = [
    ("ring", "CONV_K3S1", (1, 16, 32), [64], 64, "bf16", Exp.RING_UNIT256, "conv_ring_kernel"),                  # test_hip_ring.py BWD_SMALL
    ("skinny16", "CONV_K3S2", (2, 8, 8), [32], 64, "bf16", 0, "conv_skinny16_kernel"),                           # test_hip_sweep.py
    ("bf16", "CONV_K3S1", (2, 20, 32), [32], 64, "bf16", 0, "conv_bf16_kernel"),                                 # test_hip_sweep.py: ragged tiles
    ("mfma", "CONV_K3S2", (2, 16, 16), [32], 32, "fp32", 0, "conv_mfma_kernel<dgrad subpix k3s2>"),              # test_hip_backward.py
]


def out_extent(kname, h, w):
    if kname == "CONV_K3S2":
        return (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return (2 * h, 2 * w) if kname == "CONVT_K4S2" else (h, w)


def fwd_args(A, case, alloc):
    """pws_conv_args of a FWD_CASES row; alloc(bytes) -> a 256-byte aligned address (device memory, or a fake one for a plan)."""
    _, kname, (n, h, w), src_c, cout, mode, _, extra, _ = case
    L = A.lib()
    kind, cin, es = getattr(A, kname), sum(src_c), 2 if mode == "bf16" else 4
    oh, ow = out_extent(kname, h, w)
    a = A.PwsConvArgs()
    a.kind, a.n, a.h, a.w, a.nsrc, a.cout, a.act = kind, n, h, w, len(src_c), cout, 1
    for i, c in enumerate(src_c):
        a.src[i].ptr, a.src[i].channels, a.src[i].ld = alloc(n * h * w * c * es), c, (0 if mode == "nchw" else c)
    a.src_nchw = 1 if mode == "nchw" else 0
    a.w_packed = alloc(4 * L.pws_packed_weight_floats(kind, cin, cout))
    a.bias, a.out, a.out_ld = alloc(4 * cout), alloc(n * oh * ow * cout * es), cout
    a.ws_bytes = 64 << 20
    a.ws = alloc(a.ws_bytes)
    if mode == "bf16":
        a.math, a.store = A.MATH_BF16, A.STORE_BF16
        a.w_bf16 = alloc(4 * L.pws_packed_bf16_floats(PLANES[kname], (cin + 15) // 16 * 16, cout))
    if "wino" in extra:
        a.w_wino = alloc(4 * (L.pws_packed_wino_ct4_floats if kname == "CONVT_K4S2" else L.pws_packed_wino_floats)(cin, cout))
    if "wring" in extra:
        a.w_wring = alloc(4 * L.pws_packed_wring_floats(kind, cin, cout))
    return a


def bwd_args(A, case, alloc):
    _, kname, (n, h, w), src_c, cout, mode, _, _ = case
    L = A.lib()
    kind, cin, es = getattr(A, kname), sum(src_c), 2 if mode == "bf16" else 4
    oh, ow = out_extent(kname, h, w)
    da = A.PwsConvBwdDataArgs()
    da.kind, da.n, da.h, da.w, da.cout = kind, n, h, w, cout
    da.gout, da.gout_ld, da.ndst = alloc(n * oh * ow * cout * es), cout, len(src_c)
    da.w_dgrad = alloc(4 * L.pws_packed_dgrad_floats(kind, cin, cout))
    for i, c in enumerate(src_c):
        da.dst[i].ptr, da.dst[i].channels, da.dst[i].ld = alloc(n * h * w * c * es), c, c
    da.ws_bytes = 64 << 20
    da.ws = alloc(da.ws_bytes)
    if mode == "bf16":
        da.math, da.store = A.MATH_BF16, A.STORE_BF16
        da.w_dgrad_bf16 = alloc(4 * L.pws_packed_bf16_floats(9 if "S1" in kname else 16, cout, cin))
    return da


class FakeAlloc:
    """256-byte aligned addresses that are never dereferenced (a plan inspects pointers for NULL and alignment only)."""

    def __init__(self):
        self.at = 1 << 40

    def __call__(self, nbytes):
        p = self.at
        self.at += (int(nbytes) + 255) // 256 * 256 + 256
        return p
