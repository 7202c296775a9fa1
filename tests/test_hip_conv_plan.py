"""Plan equals launch: what the dispatch ladder reports without launching (pws_netg_forward_plan, pws_conv2d_fwd_plan,
pws_conv2d_bwd_data_plan, called with the device's CU count) is what a profiled launch records -- for whole eager forwards of the
generator (layer tag and kernel per conv launch, in issue order) and for one single call per kernel family (tests/conv_plan_cases.py)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

# the conv launches' ids (include/pwstable.h: pws_prof_kernel_name): everything else a forward records is a head, a conversion or a pass
CONV_KERNELS = ("conv_mfma_kernel", "conv_bf16_kernel", "conv_ring_kernel", "conv_ringf_kernel", "wino_ring_kernel", "wino_k3s1_kernel",
                "wino_ct4_kernel", "conv_skinny_kernel", "conv_skinny16_kernel", "conv_first_kernel", "wino5_first_kernel")


def device_cus(A):
    cus, is950 = ctypes.c_int(0), ctypes.c_int(0)
    A.check(A.lib().pws_device_info(ctypes.byref(cus), ctypes.byref(is950)), "pws_device_info")
    return cus.value


class DeviceAlloc:
    def __init__(self):
        self.keep = []

    def __call__(self, nbytes):
        t = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")
        self.keep.append(t)
        return t.data_ptr()


@pytest.mark.parametrize("n,ngf,math,store,training", [(8, 64, "fp32", "fp32", 0), (8, 64, "bf16", "bf16", 0), (2, 16, "fp32", "fp32", 1)])
def test_forward_plan_equals_profiled_forward(hip, n, ngf, math, store, training):
    A = hip
    L, st = A.lib(), A.current_stream()
    opts = A.PwsNetgOpts(A.MATH_BF16 if math == "bf16" else A.MATH_FP32, A.STORE_BF16 if store == "bf16" else A.STORE_FP32, 1, 0, 0)
    buf = (A.PwsConvChoice * 256)()
    cnt = L.pws_netg_forward_plan(n, 31, ngf, training, ctypes.byref(opts), device_cus(A), buf, 256)
    assert 40 < cnt <= 256, L.pws_last_error()
    plan = [(buf[i].tag, L.pws_prof_kernel_name(buf[i].kernel_id).decode()) for i in range(cnt)]
    # an eager forward on zero weights and a zero window: the dispatch does not look at values
    packed = torch.zeros(L.pws_netg_packed_floats(31, ngf), device="cuda")
    x = torch.zeros((n, 31, 256, 256), device="cuda")
    ws_bytes = L.pws_netg_workspace_bytes(n, 31, ngf, training)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    grids, resid = torch.empty((3, n, 256, 256, 2), device="cuda"), torch.empty((3, n, 256, 256, 2), device="cuda")
    thetas = torch.empty((3, n, 6), device="cuda")
    torch.cuda.synchronize()
    L.pws_prof_enable(1)
    try:
        A.check(L.pws_netg_forward_opts(A.ptr(packed), A.ptr(x), n, 31, ngf, training, 0, A.ptr(ws), ws_bytes, A.ptr(grids), A.ptr(resid), A.ptr(thetas),
                                        ctypes.byref(opts), st),
                "pws_netg_forward_opts")
        torch.cuda.synchronize()
        recs = A.prof_collect(4096)
    finally:
        L.pws_prof_enable(0)
    ran = [(tag, name) for name, tag, _, _, _ in recs if name.startswith(CONV_KERNELS)]
    assert ran == plan


def _profiled(A, call):
    L = A.lib()
    torch.cuda.synchronize()
    L.pws_prof_enable(1)
    try:
        call()
        torch.cuda.synchronize()
        return [r[0] for r in A.prof_collect()]
    finally:
        L.pws_prof_enable(0)


@pytest.mark.parametrize("case", C.FWD_CASES, ids=[c[0] for c in C.FWD_CASES])
def test_single_forward_plan_equals_launch(hip, case):
    A = hip
    L, st = A.lib(), A.current_stream()
    alloc = DeviceAlloc()
    a = C.fwd_args(A, case, alloc)
    c = A.PwsConvChoice()
    *_, exp, _, kernel = case
    with A.experiment(exp):
        A.check(L.pws_conv2d_fwd_plan(ctypes.byref(a), device_cus(A), ctypes.byref(c)), "pws_conv2d_fwd_plan")
        names = _profiled(A, lambda: A.check(L.pws_conv2d_fwd(ctypes.byref(a), st), "pws_conv2d_fwd"))
    assert names == [L.pws_prof_kernel_name(c.kernel_id).decode()] == [kernel], (names, c.as_dict(L))


@pytest.mark.parametrize("case", C.BWD_CASES, ids=[c[0] for c in C.BWD_CASES])
def test_single_data_gradient_plan_equals_launch(hip, case):
    A = hip
    L, st = A.lib(), A.current_stream()
    alloc = DeviceAlloc()
    da = C.bwd_args(A, case, alloc)
    c = A.PwsConvChoice()
    *_, exp, kernel = case
    with A.experiment(exp):
        A.check(L.pws_conv2d_bwd_data_plan(ctypes.byref(da), device_cus(A), ctypes.byref(c)), "pws_conv2d_bwd_data_plan")
        names = _profiled(A, lambda: A.check(L.pws_conv2d_bwd_data(ctypes.byref(da), st), "pws_conv2d_bwd_data"))
    assert names == [L.pws_prof_kernel_name(c.kernel_id).decode()] == [kernel], (names, c.as_dict(L))
