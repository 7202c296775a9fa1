"""conv_ringf_kernel's stride-2 workgroup shapes give the same bits (csrc/conv_ring_f32.hip, conv_ringf_try).

The product runs launches of 8 x 32 tiles as half workgroups (two per CU) and 16 x 32 tiles as full ones.  PWS_OPT_EXPERIMENT 2216
forces full workgroups everywhere (the previous product), 2232 half workgroups everywhere.  Every variant walks the same K groups in the
same order for each output pixel with the same matrix instruction, so the outputs must be bit-identical; the product itself is checked
against the C oracle in tests/test_hip_ops.py::test_fp32_ring_kernel_vs_oracle.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from pwstablenet_amd.hipabi import Exp  # noqa: E402
pytestmark = pytest.mark.gpu

# (N, H, W, cin, cout) of the input; the launch picks 16 x 32 tiles, 8 x 32 tiles, or 8 x 32 tiles of 32 output channels
CASES = [(8, 256, 256, 64, 64), (4, 256, 256, 64, 64), (8, 64, 64, 128, 256), (8, 128, 128, 96, 128)]


def run_k3s2(A, n, h, w, cin, cout, exp):
    L, st = A.lib(), A.current_stream()
    g = torch.Generator().manual_seed(n * 1000 + cin + cout)
    wt = (torch.randn((cout, cin, 3, 3), generator=g) / (9 * cin) ** 0.5).cuda()
    x = torch.randn((n, h, w, cin), generator=g).cuda()
    b = torch.randn(cout, generator=g).cuda()
    wp = torch.empty(L.pws_packed_weight_floats(A.CONV_K3S2, cin, cout), device="cuda")
    A.check(L.pws_pack_conv_weight(A.ptr(wt), A.ptr(wp), A.CONV_K3S2, cin, cout, st), "pack")
    out = torch.full((n, h // 2, w // 2, cout), float("nan"), device="cuda")
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    a = A.PwsConvArgs()
    a.kind, a.n, a.h, a.w, a.nsrc, a.cout, a.act = A.CONV_K3S2, n, h, w, 1, cout, 1
    a.src[0].ptr, a.src[0].channels, a.src[0].ld = x.data_ptr(), cin, cin
    a.w_packed, a.bias, a.out, a.out_ld, a.ws, a.ws_bytes = wp.data_ptr(), b.data_ptr(), out.data_ptr(), cout, ws.data_ptr(), ws.numel()
    try:
        with A.experiment(exp):
            L.pws_prof_enable(1)
            A.check(L.pws_conv2d_fwd(ctypes.byref(a), st), "conv")
            L.pws_prof_enable(0)
            names = [r[0] for r in A.prof_collect()]
    finally:
        L.pws_prof_enable(0)
    torch.cuda.synchronize()
    return out.cpu().numpy(), names


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_%dx%d_%d_%d" % c)
def test_k3s2_workgroup_variants_bit_identical(hip, case):
    ref, names = run_k3s2(hip, *case, 0)
    assert names == ["conv_ringf_kernel"], names
    assert not np.isnan(ref).any()
    for exp in (Exp.RINGF_VARIANT + 16, Exp.RINGF_VARIANT + 32):
        got, names = run_k3s2(hip, *case, exp)
        assert names == ["conv_ringf_kernel"], (exp, names)
        assert got.tobytes() == ref.tobytes(), (exp, float(np.abs(got - ref).max()))
