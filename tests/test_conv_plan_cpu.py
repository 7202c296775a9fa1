"""The conv dispatch ladder read off without a GPU (csrc/conv_dispatch.hip through pws_conv2d_fwd_plan, pws_conv2d_bwd_data_plan and
pws_netg_forward_plan): the plan entry points run on a machine without a device -- which is what keeps every family's plan step free of
HIP calls --, the decisions of the pinned configurations equal tests/golden/conv_dispatch.json field by field (a pull request that
moves a threshold regenerates it with tools/conv_plan_table.py --write and shows the diff), and what other code assumes about the
ladder's outcome holds: the bf16 generator never lands on a family that reads fp32 weights; ngf 16 lands its odd layers on
conv_mfma_kernel."""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "tools")]
import conv_plan_cases as C  # noqa: E402
import conv_plan_table as T  # noqa: E402

CUS = 256
# what each family reads: the bf16 families take pws_conv_args.w_bf16 / pws_conv_bwd_data_args.w_dgrad_bf16, every other one the fp32
# w_packed / w_wino / w_wring (forward) or w_dgrad (data gradient)
BF16_FAMILIES = {"conv_ring_kernel", "conv_skinny16_kernel", "conv_bf16_kernel"}


@pytest.fixture(scope="module")
def A():
    from pwstablenet_amd import build, hipabi
    build.build(verbose=False)
    return hipabi


def plan_fwd(A, args, cus=CUS):
    c = A.PwsConvChoice()
    rc = A.lib().pws_conv2d_fwd_plan(ctypes.byref(args), cus, ctypes.byref(c))
    assert rc == 0, A.lib().pws_last_error()
    return c.as_dict(A.lib())


def plan_bwd(A, args, cus=CUS):
    c = A.PwsConvChoice()
    rc = A.lib().pws_conv2d_bwd_data_plan(ctypes.byref(args), cus, ctypes.byref(c))
    assert rc == 0, A.lib().pws_last_error()
    return c.as_dict(A.lib())


def test_golden_table(A):
    """Kernel, variant, grid, workgroup, LDS, K split and follow-up pass of every conv launch of the pinned configurations at 256 CUs."""
    with open(T.GOLDEN) as f:
        want = json.load(f)
    assert want["_meta"]["compute_units"] == T.GOLDEN_CUS and set(want["configs"]) == set(T.PINNED)
    for name, cfg in T.PINNED.items():
        got = T.forward_plan(*cfg)
        assert len(got) == len(want["configs"][name]), name
        for i, (g, w) in enumerate(zip(got, want["configs"][name])):
            for field in ("tag", "kernel", "variant", "grid", "threads", "lds_bytes", "ksplit", "follow"):
                assert g[field] == w[field], (name, i, field, g, w)


@pytest.mark.parametrize("case", C.FWD_CASES, ids=[c[0] for c in C.FWD_CASES])
def test_single_forward_call_plans_without_a_device(A, case):
    *_, exp, _, kernel = case
    with A.experiment(exp):
        got = plan_fwd(A, C.fwd_args(A, case, C.FakeAlloc()))
    assert got["kernel"] == kernel, got
    assert got["threads"] > 0 and got["grid"][0] > 0 and got["ksplit"] >= 1


@pytest.mark.parametrize("case", C.BWD_CASES, ids=[c[0] for c in C.BWD_CASES])
def test_single_data_gradient_call_plans_without_a_device(A, case):
    *_, exp, kernel = case
    with A.experiment(exp):
        got = plan_bwd(A, C.bwd_args(A, case, C.FakeAlloc()))
    assert got["kernel"] == kernel, got


def test_plan_keeps_the_argument_checks(A):
    L = A.lib()
    c = A.PwsConvChoice()
    assert L.pws_conv2d_fwd_plan(None, CUS, ctypes.byref(c)) == -22 and b"NULL" in L.pws_last_error()
    assert L.pws_conv2d_bwd_data_plan(None, CUS, ctypes.byref(c)) == -22
    a = C.fwd_args(A, C.FWD_CASES[10], C.FakeAlloc())
    assert L.pws_conv2d_fwd_plan(ctypes.byref(a), 0, ctypes.byref(c)) == -22
    a.src[0].ptr += 4   # a misaligned source is refused by the plan as by the launch
    assert L.pws_conv2d_fwd_plan(ctypes.byref(a), CUS, ctypes.byref(c)) == -22 and b"16-B aligned" in L.pws_last_error()
    assert L.pws_netg_forward_plan(8, 31, 60, 0, None, CUS, None, 0) == -22   # ngf must be a multiple of 16
    assert L.pws_netg_forward_plan(8, 31, 64, 0, None, CUS, None, 0) > 40      # counting only


# ---- what other code assumes about the ladder's outcome
BF16_GRID = [(ngf, n, tr) for ngf in (32, 64) for n in (1, 2, 8, 16, 64) for tr in (0, 1)]


@pytest.mark.parametrize("ngf,n,training", BF16_GRID)
def test_bf16_forward_never_reads_fp32_weights(A, ngf, n, training):
    """bf16 math + bf16 storage: no conv layer of the forward is planned onto a family that reads w_packed, w_wino or w_wring.  This is
    what pws_netg_pack_weights_train relies on when it writes no fp32 copies, pws_netg_pack_weights_for(math = bf16) when it leaves out
    the Winograd copies, and Exec::run_conv when it hands the ladder no Winograd pointers."""
    rows = T.forward_plan(n, ngf, "bf16", "bf16", training)
    assert len(rows) > 40
    wrong = [(r["tag"], r["kernel"]) for r in rows if r["kernel"] not in BF16_FAMILIES]
    assert not wrong, wrong


def generator_dgrad_calls(A, n, ngf):
    """The data-gradient calls of the generator's backward with bf16 math and storage, one per conv layer that has one: shapes from the
    layer table (spec.layer_specs gives kinds and channels; the input extent follows from the level), at batch n and 2 n, the
    destinations as one tensor (how a virtual concat splits them does not enter the families' coverage at these channel counts)."""
    from pwstablenet_amd.spec import layer_specs
    kinds = {(3, 1, "conv"): "CONV_K3S1", (3, 2, "conv"): "CONV_K3S2", (3, 1, "convT"): "CONVT_K3S1", (4, 2, "convT"): "CONVT_K4S2"}
    # input edge of each layer at the 256 x 256 window: layer index -> edge (csrc/netg_layers.h's order)
    edge = {}
    for i in range(7):
        edge[1 + i] = 256 >> i           # down1..7: stride-2 convs from 256 .. 4
        edge[8 + i] = 2 << i             # up7..1: transposed convs from 2 .. 128
        edge[16 + 2 * i] = 256 >> i      # down_bottom k conv_same
        edge[17 + 2 * i] = 256 >> i      # ... mpconv (stride 2)
        edge[30 + 2 * i] = 2 << i        # up_bottom mpconv (transposed, from the level below)
        edge[31 + 2 * i] = 2 << i        # ... conv_same at that level
    calls = []
    for i, ls in enumerate(layer_specs(31, 2, ngf)):
        if i not in edge:
            continue
        kname = kinds[(ls.k, ls.s, ls.kind)]
        for batch in (n, 2 * n):   # (stages 2 and 3 run as one launch of twice the batch)
            calls.append((i, C.bwd_args(A, ("l%d" % i, kname, (batch, edge[i], edge[i]), [ls.cin], ls.cout, "bf16", 0, None), C.FakeAlloc())))
    return calls


@pytest.mark.parametrize("ngf,n", [(ngf, n) for ngf in (32, 64) for n in (1, 2, 8, 16, 64)])
def test_bf16_data_gradient_never_reads_fp32_weights(A, ngf, n):
    """Same conditions, data gradient: no layer is planned onto a family that reads the fp32 w_dgrad."""
    calls = generator_dgrad_calls(A, n, ngf)
    assert len(calls) == 2 * 42
    wrong = []
    for i, da in calls:
        got = plan_bwd(A, da)
        if got["kernel"] not in BF16_FAMILIES:
            wrong.append((i, got["kernel"]))
    assert not wrong, wrong


def test_ngf16_odd_layers_fall_through_to_the_direct_kernel(A):
    """ngf 16 with bf16 math: a layer with a source that is no multiple of 32 channels is declined by the bf16 kernels and, as the
    comment in Exec::run_conv says, runs on conv_mfma_kernel over w_packed -- not on a Winograd kernel, whose weights
    pws_netg_pack_weights_for(math = bf16) did not pack when the layer has bf16 weights."""
    from pwstablenet_amd.spec import layer_specs
    specs = layer_specs(31, 2, 16)
    for n in (2, 8):
        rows = T.forward_plan(n, 16, "bf16", "fp32", 1)
        fell = [r for r in rows if r["kernel"] not in BF16_FAMILIES and r["tag"] != 0]
        assert fell, "ngf 16 has layers the bf16 kernels decline"
        for r in fell:
            has_bf16_weights = ((specs[r["tag"]].cin + 15) // 16 * 16) % 32 == 0
            if has_bf16_weights:   # declined with bf16 weights packed: only the direct kernel may take it
                assert r["kernel"].startswith("conv_mfma_kernel"), r
