"""Fused Adam (csrc/adam.hip) against float64: through the C ABI (pws_adam_step_d, pws_adam_step_multi_d and the float entries) and
through optim.Adam on its own state layout.  p, m AND v are judged, every time, at step counts from 1 to 100 000 and over consecutive
steps with the state carried on the device.

The truth is tests/adam_ref64.py (float64 numpy, torch's formulation, the hyper-parameters as the doubles the caller wrote; held to
torch's float64 Adam by tests/test_adam_ref64_cpu.py, which also puts a numpy restatement of the kernels through every case below).  The
yardstick is torch.optim.Adam(foreach=False) in fp32 on the CPU from the same state.  The rule is the project's (Figures of
tests/test_hip_objective_float64.py): on each judged tensor

    kernel error  <=  4 x torch-fp32 error  +  4 fp32 ulps of the tensor's largest float64 magnitude          (max over the tensor)

Two conditions keep the max-norm from hiding errors.  p starts at zero (or within 1e-3 lr of it), so the judged p is the displacement --
next to a p ~ 1 a whole update is a few thousand ulps and its error none.  And gradients of different magnitude are separate tensors:
one judge call per magnitude class.  The only other bounds are 2^-126 for a sub-normal v (met whether or not the device keeps fp32
denormals) and == on bits for the outcomes that are exact.  No element is excluded anywhere.

With 1.f - (float)beta2 formed on the device (the kernels before pws_adam_step_d) v misses its bound wherever it is made of
(1 - beta2) g^2 terms -- 23-fold in (a) from zero moments, 20-fold in (b), 30-fold in (h), 22-fold in (i) -- and p misses it 12-fold in (a),
7-fold in (b), 8-fold in (e), 4-fold in (f), 19-fold in (h), 9-fold in (i) (measured on an MI355X; the numpy restatement of
tests/test_adam_ref64_cpu.py gives the same figures).  (g) found that the scalar and the float4 paths rounded v differently.

In brackets in the tests' docstrings: kernel error / torch-fp32 error measured on an MI355X, per judged kind of tensor at the row that
used the largest share of its bound, and that share."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref64 as R  # noqa: E402
from test_hip_objective_float64 import Figures  # noqa: E402  (the rule itself: FACTOR = 4, ULPS = 4)

pytestmark = pytest.mark.gpu

DEV = "cuda"
T = torch.from_numpy
EINVAL = -22


def dev(a):
    """a fresh allocation (torch's are 512-byte aligned)"""
    return T(np.ascontiguousarray(a)).to(DEV)


def offset_view(a, floats):
    """the same values `floats` * 4 bytes into an allocation of their own"""
    buf = torch.zeros(a.size + 4, device=DEV)
    view = buf[floats:floats + a.size]
    view.copy_(T(np.ascontiguousarray(a)))
    assert view.data_ptr() % 16 == (4 * floats) % 16
    return view


def single(hip, p, g, m, v, hyper, step, entry="pws_adam_step_d"):
    return getattr(hip.lib(), entry)(hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v), p.numel(), *hyper, step, hip.current_stream())


def multi(hip, ps, gs, ms, vs, hyper, step, counts=None, entry="pws_adam_step_multi_d"):
    """counts: given where the table holds empty entries (their tensors are None: NULL pointers)"""
    n = len(ps)
    arr = lambda ts: (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    counts = (ctypes.c_size_t * n)(*(counts if counts is not None else [t.numel() for t in ps]))
    return getattr(hip.lib(), entry)(arr(ps), arr(gs), arr(ms), arr(vs), counts, n, *hyper, step, hip.current_stream())


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def judge3(fig, tag, got, ref, t32):
    for name, a, b, c in zip("pmv", got, ref, t32):
        fig.judge(("%s %s" % (tag, name)).strip(), a.reshape(-1), T(np.ascontiguousarray(b)).reshape(-1), T(np.ascontiguousarray(c)).reshape(-1))


# ------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("state", ["given", "zero"])
@pytest.mark.parametrize("hyper", R.HYPERS, ids=lambda h: "lr%g-b%g-%g-eps%g" % h)
def test_one_step_vs_float64(hip, hyper, state):
    """(a) One step at step counts 1, 2, 3, 10, 1000, 100 000 from moments m ~ 0.1 N(0,1) s, v ~ U(0,1) s^2 with g ~ N(0,1) s, one tensor
    of 4099 elements per s in {1e-15, 1e-8, 1e-4, 1, 1e4, 1e15} (sqrt(v) below, at and far above eps), and from zero moments (s from
    1e-8: there v is (1 - beta2) g^2 alone, the term the fp32 complement got wrong).  The six tensors go through pws_adam_step_multi_d in
    one call and through pws_adam_step_d one by one; the two must agree bit for bit, and p, m, v of every class are judged.
    [at the largest share of a bound: p 3.7e-09 / 1.7e-09, share 0.26 (step 100 000, s = 1e-4); m 3.1e-12 / 2.8e-12, share 0.12; v 1.2e-09 /
    1.2e-09, share 0.14; largest kernel / torch-fp32 ratio 2.2]"""
    fig = Figures("adam one step %s %s:" % (state, hyper))
    for step in R.STEPS:
        cases = R.one_step_classes(state)
        one = [[dev(c[k]) for k in "pgmv"] for c in cases]
        many = [[dev(c[k]) for k in "pgmv"] for c in cases]
        for t in one:
            hip.check(single(hip, *t, hyper, step), "pws_adam_step_d")
        hip.check(multi(hip, *[[t[k] for t in many] for k in range(4)], hyper, step), "pws_adam_step_multi_d")
        for c, a, b in zip(cases, one, many):
            assert all(same_bits(a[k], b[k]) for k in (0, 2, 3)) and same_bits(b[1], dev(c["g"])), (step, c["scale"])
            args = (c["p"], c["g"], c["m"], c["v"]) + hyper + (step,)
            judge3(fig, "step %d s %g" % (step, c["scale"]), (b[0], b[2], b[3]), R.step(*args), R.torch32(*args))
    fig.finish()


# ------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("hyper", R.HYPERS[:2], ids=lambda h: "lr%g-b%g-%g-eps%g" % h)
def test_fifty_steps_vs_float64(hip, hyper):
    """(b) Fifty consecutive steps from p = m = v = 0, the state carried on the device, in float64 and in torch's fp32 optimiser, all three
    driven by the same fp32 gradients, whose scale changes from step to step over four decades.  p, m, v after steps 1, 2, 10 and 50.
    [after 50 steps: p 1.1e-09 / 6.9e-10, share 0.30; m 4.0e-07 / 1.9e-07, share 0.32; v 4.3e-07 / 4.3e-07, share 0.22]"""
    grads = R.run_gradients()
    z = [np.zeros(R.RUN_N, np.float32)]
    r64, t32 = R.run64(z, [[g] for g in grads], hyper), R.run_torch32(z, [[g] for g in grads], hyper)
    p, m, v = dev(z[0]), dev(z[0]), dev(z[0])
    fig = Figures("adam 50 steps %s:" % (hyper,))
    for t, g in enumerate(grads, 1):
        hip.check(multi(hip, [p], [dev(g)], [m], [v], hyper, t), "pws_adam_step_multi_d")
        if t in R.RUN_JUDGED:
            judge3(fig, "step %d" % t, (p, m, v), r64[t - 1][0], t32[t - 1][0])
    fig.finish()


# ------------------------------------------------------------------------------------------------------------ (c)
def _both_entries(hip, c, hyper, step):
    """[(p, m, v) of the single entry, (p, m, v) of the multi entry] on fresh copies of a case"""
    out = []
    for call in (lambda t: single(hip, *t, hyper, step), lambda t: multi(hip, *[[x] for x in t], hyper, step)):
        t = [dev(c[k]) for k in "pgmv"]
        hip.check(call(t), "adam")
        out.append((t[0], t[2], t[3]))
    return out


def test_exact_outcomes(hip):
    """(c) Outcomes that are exact, compared with == on bits, both entries, p0 ~ N(0,1), 4099 elements.
    g = 0 on m = v = 0: p keeps its bits, m and v stay +0.
    |g| = 1e30: g^2 overflows, v = +inf everywhere, m / inf = 0 and p keeps its bits; m is finite and is judged by the rule.
    A NaN gradient at elements 1 (inside a float4) and 4098 (the scalar tail): p, m, v are NaN there and nowhere else, and every other
    element has the bits of the same step on the gradients without the NaNs (the kernels are element-wise).
    [m under |g| = 1e30: kernel 0 / torch-fp32 0: both round float64's m exactly]"""
    hyper, step = R.HYPERS[0], 3
    c = R.moment_case(R.N_CLASS, 1.0, 400, state="zero", p0="normal")
    c["g"][:] = 0
    for p, m, v in _both_entries(hip, c, hyper, step):
        assert same_bits(p, dev(c["p"])) and same_bits(m, dev(c["m"])) and same_bits(v, dev(c["v"]))

    c = R.moment_case(R.N_CLASS, 1.0, 401, p0="normal")
    c["g"] = np.where(c["g"] > 0, 1e30, -1e30).astype(np.float32)
    args = (c["p"], c["g"], c["m"], c["v"]) + hyper + (step,)
    ref, t32 = R.step(*args), R.torch32(*args)
    fig = Figures("adam |g| = 1e30:")
    for tag, (p, m, v) in zip(("single", "multi"), _both_entries(hip, c, hyper, step)):
        assert same_bits(p, dev(c["p"])) and same_bits(v, torch.full_like(v, float("inf")))
        fig.judge(tag + " m", m, T(ref[1]), T(t32[1]))
    fig.finish()

    c = R.moment_case(R.N_CLASS, 1.0, 402, p0="normal")
    clean = _both_entries(hip, c, hyper, step)
    nans = [1, R.N_CLASS - 1]
    c["g"][nans] = np.nan
    mask = torch.zeros(R.N_CLASS, dtype=torch.bool, device=DEV)
    mask[nans] = True
    for got, want in zip(_both_entries(hip, c, hyper, step), clean):
        for a, b in zip(got, want):
            assert torch.equal(torch.isnan(a), mask) and same_bits(a[~mask], b[~mask])


# ------------------------------------------------------------------------------------------------------------ (d)
def test_subnormal_v(hip):
    """(d) s = 1e-20: g^2 ~ 1e-40 and v ~ U(0,1) 1e-40 lie below 2^-126, every float64 v of the case does.  p and m by the rule (sqrt(v) is
    far below eps, so p does not depend on what became of v); v within 2^-126 of float64, which holds for a device that keeps fp32
    denormals and for one that flushes them.
    [the MI355X keeps them: all 4099 v are non-zero denormals, off by at most 1.4e-45, one step of the denormal grid; p 2.0e-22 / 2.6e-22,
    share 0.11; m 8.1e-28 / 8.1e-28, share 0.083]"""
    hyper, step = R.HYPERS[0], 2
    c = R.moment_case(R.N_CLASS, R.SUBNORMAL_SCALE, 200)
    args = (c["p"], c["g"], c["m"], c["v"]) + hyper + (step,)
    ref, t32 = R.step(*args), R.torch32(*args)
    assert ref[2].max() < R.TINY32
    fig = Figures("adam sub-normal v:")
    for tag, (p, m, v) in zip(("single", "multi"), _both_entries(hip, c, hyper, step)):
        judge3(fig, tag, (p, m), ref[:2], t32[:2])
        fig.judge_abs(tag + " v", float((v.double().cpu() - T(ref[2])).abs().max()), R.TINY32)
        kept = int((v != 0).sum())
        print("adam sub-normal v (%s): %d of %d results are non-zero denormals: the device %s fp32 denormals" %
              (tag, kept, v.numel(), "KEEPS" if kept else "FLUSHES"))
    fig.finish()


# ------------------------------------------------------------------------------------------------------------ (e)
def test_grid_stride_second_trip(hip):
    """(e) pws_adam_step_d on 2048 * 256 * 4 + 1024 + 3 elements: its grid is capped at 2048 workgroups of 256 float4 lanes, so the first 256
    lanes take a second trip of the grid-stride loop and three elements are left to the scalar tail.  Judged by the rule, and equal bit
    for bit to pws_adam_step_multi_d (one workgroup per 4096 elements, no loop) on the same data.
    [p 2.6e-10 / 1.7e-10, share 0.16; m 1.2e-07 / 1.7e-07, share 0.073; v 1.0e-07 / 1.0e-07, share 0.11]"""
    hyper, step = R.HYPERS[0], 3
    c = R.moment_case(R.GRID_STRIDE_COUNT, 1.0, 300)
    args = (c["p"], c["g"], c["m"], c["v"]) + hyper + (step,)
    (p, m, v), other = _both_entries(hip, c, hyper, step)
    assert all(same_bits(a, b) for a, b in zip((p, m, v), other))
    fig = Figures("adam grid-stride %d:" % R.GRID_STRIDE_COUNT)
    judge3(fig, "", (p, m, v), R.step(*args), R.torch32(*args))
    fig.finish()


# ------------------------------------------------------------------------------------------------------------ (f)
def test_block_table(hip):
    """(f) pws_adam_step_multi_d on 100 tensors with counts 1, 3, 4, 4095, 4096, 4097, 8192, 8193 repeated and count 0 with NULL pointers
    at positions 0, 47, 48, 99: two launches of 48 tensors each (the empty entries skipped before and inside the first table), and a
    last pass that finds nothing to launch.  All elements as one tensor (one magnitude class) by the rule, and every tensor bit for bit
    against its own pws_adam_step_d call.
    [p 2.3e-10 / 1.8e-10, share 0.14; m 1.2e-07 / 1.7e-07, share 0.071; v 1.0e-07 / 1.0e-07, share 0.12]"""
    hyper, step = R.HYPERS[0], 3
    c = R.table_case()
    cut = lambda a: [dev(a[lo:hi]) if hi > lo else None for lo, hi in zip(c["offsets"], c["offsets"][1:])]  # noqa: E731
    many, one = [cut(c[k]) for k in "pgmv"], [cut(c[k]) for k in "pgmv"]
    hip.check(multi(hip, *many, hyper, step, counts=c["counts"]), "pws_adam_step_multi_d")
    for t in zip(*one):
        if t[0] is not None:
            hip.check(single(hip, *t, hyper, step), "pws_adam_step_d")
    for k in (0, 2, 3):
        assert all(a is None or same_bits(a, b) for a, b in zip(many[k], one[k])), "pmv"[k - (k > 0)]
    assert all(a is None or same_bits(a, b) for a, b in zip(many[1], cut(c["g"])))
    args = (c["p"], c["g"], c["m"], c["v"]) + hyper + (step,)
    fig = Figures("adam block table:")
    judge3(fig, "", [torch.cat([t for t in many[k] if t is not None]) for k in (0, 2, 3)], R.step(*args), R.torch32(*args))
    fig.finish()


# ------------------------------------------------------------------------------------------------------------ (g)
# floats of offset of (p, g, m, v) into their allocations: only p unaligned, only g, all four (mixed), none, all four by 8 bytes
UNALIGNED = [(4099, (1, 0, 0, 0)), (4096, (0, 2, 0, 0)), (257, (1, 2, 1, 2)), (8193, (0, 0, 0, 0)), (5, (2, 2, 2, 2))]


def test_unaligned_pointers(hip):
    """(g) The scalar path of adam_multi_kernel (a tensor any of whose four pointers is not 16-byte aligned): the same values as views 4
    and 8 bytes into their allocations give the bits of the aligned run, for the double and the float entry.  pws_adam_step_d takes
    unaligned buffers up to 256 elements (one lane each) and gives the aligned bits; 257 elements are refused (PWS_EINVAL, "16-byte
    aligned") and nothing is written."""
    step = 3
    for entry, entry1, hyper in (("pws_adam_step_multi_d", "pws_adam_step_d", R.HYPERS[0]), ("pws_adam_step_multi", "pws_adam_step", R.HYPERS[1])):
        cases = [R.moment_case(n, 1.0, 500 + i, p0="normal") for i, (n, _) in enumerate(UNALIGNED)]
        want = [[dev(c[k]) for c in cases] for k in "pgmv"]
        got = [[offset_view(c[k], off[j]) for c, (_, off) in zip(cases, UNALIGNED)] for j, k in enumerate("pgmv")]
        hip.check(multi(hip, *want, hyper, step, entry=entry), entry)
        hip.check(multi(hip, *got, hyper, step, entry=entry), entry)
        for k in range(4):
            assert all(same_bits(a, b) for a, b in zip(got[k], want[k])), (entry, k)

        c = R.moment_case(256, 1.0, 510, p0="normal")
        want, got = [dev(c[k]) for k in "pgmv"], [offset_view(c[k], 1 + j % 2) for j, k in enumerate("pgmv")]
        hip.check(single(hip, *want, hyper, step, entry=entry1), entry1)
        hip.check(single(hip, *got, hyper, step, entry=entry1), entry1)
        assert all(same_bits(a, b) for a, b in zip(got, want)), entry1

        c = R.moment_case(257, 1.0, 511, p0="normal")
        got = [offset_view(c[k], 1) for k in "pgmv"]
        assert single(hip, *got, hyper, step, entry=entry1) == EINVAL and b"16-byte aligned" in hip.lib().pws_last_error()
        torch.cuda.synchronize()
        assert all(same_bits(a, dev(c[k])) for a, k in zip(got, "pgmv")), entry1


# ------------------------------------------------------------------------------------------------------------ (h)
def _params(p0):
    return [torch.nn.Parameter(dev(p)) for p in p0]


def _set_grads(ps, gs, has_grad=lambda i: True, transposed=()):
    for i, (p, g) in enumerate(zip(ps, gs)):
        if not has_grad(i):
            p.grad = None
        elif i in transposed:
            p.grad = dev(g.T).t()
            assert not p.grad.is_contiguous() and p.grad.shape == p.shape
        else:
            p.grad = dev(g)


def test_class_on_its_own_state_layout(hip):
    """(h) optim.Adam on 9 parameters of 1, 63, 64, 65, 4097, 105, 8192, 2 and 100 003 elements (the 64-float rounding of the moment views
    on both sides) for 12 steps; gradients are assigned to .grad, those of the (512, 16) parameter as transposed views.  After steps 1,
    2 and 12 every parameter's p and, read through opt.state[p], m and v are judged by the rule against torch.optim.Adam on CPU copies.
    Every moment has its parameter's shape, every p._version advances at every step, the views do not overlap, and no element of the
    flat buffers outside the views has changed from zero.
    [at the largest share of a bound: p 1.3e-10 / 1.2e-11, share 0.25 (step 2, the one-element parameter: one ulp); m 2.2e-07 / 2.6e-07,
    share 0.11; v 2.0e-08 / 2.0e-08, share 0.18]"""
    from pwstablenet_amd.optim import Adam
    hyper = R.HYPERS[0]
    lr, b1, b2, eps = hyper
    p0, grads = R.class_case(lr=lr)
    r64, t32 = R.run64(p0, grads, hyper), R.run_torch32(p0, grads, hyper)
    ps = _params(p0)
    opt = Adam(ps, lr=lr, betas=(b1, b2), eps=eps)
    fig = Figures("adam class:")
    for t, gs in enumerate(grads, 1):
        _set_grads(ps, gs, transposed=(R.CLASS_TRANSPOSED,))
        before = [p._version for p in ps]
        opt.step()
        assert all(p._version > b for p, b in zip(ps, before)), t
        if t in R.CLASS_JUDGED:
            for i, p in enumerate(ps):
                m, v = opt.state[p]
                assert m.shape == v.shape == p.shape
                judge3(fig, "step %d param %d" % (t, i), (p.detach(), m, v), r64[t - 1][i], t32[t - 1][i])
    fig.finish()
    (flat_m, flat_v), = opt.flat.values()
    for flat, k in ((flat_m, 0), (flat_v, 1)):
        used = torch.zeros(flat.numel(), dtype=torch.int32, device=DEV)
        for p in ps:
            off = (opt.state[p][k].data_ptr() - flat.data_ptr()) // 4
            assert 0 <= off and off + p.numel() <= flat.numel() and off % 64 == 0
            used[off:off + p.numel()] += 1
        assert int(used.max()) == 1 and int(used.sum()) == sum(R.CLASS_NUMELS) and flat.numel() == sum((n + 63) // 64 * 64 for n in R.CLASS_NUMELS)
        assert not bool(flat[used == 0].any())


# ------------------------------------------------------------------------------------------------------------ (i)
def test_late_joiner(hip):
    """(i) Of three parameters one has .grad = None in steps 1 to 3 and a gradient from step 4: it is left alone until then and then takes
    ITS first step (torch's bias corrections of step 1, not of step 4: a factor 1.07 in p with beta1 = 0.5, or 1 / (1 - beta1^4)).
    Another is made on the device after the optimiser and goes through the zeros_like fallback of step().  All three by the rule
    after steps 4 and 6 against torch.optim.Adam, which counts steps per parameter.
    [p 7.8e-10 / 6.3e-10, share 0.18; m 7.2e-08 / 7.2e-08, share 0.094; v 1.7e-09 / 1.7e-09, share 0.16.  With one global step count the
    late parameter's p was off by 6.6e-05 at step 4: 48 000 times its bound]"""
    from pwstablenet_amd.optim import Adam
    hyper = R.HYPERS[0]
    lr, b1, b2, eps = hyper
    p0, grads, has_grad = R.join_case()
    r64, t32 = R.run64(p0, grads, hyper, has_grad), R.run_torch32(p0, grads, hyper, has_grad)
    ps = _params(p0[:2])
    opt = Adam(ps, lr=lr, betas=(b1, b2), eps=eps)
    ps.append(torch.nn.Parameter(dev(p0[2])))            # made after the optimiser: no view of the flat buffers for it
    opt.params.append(ps[2])
    fig = Figures("adam late joiner:")
    for t, gs in enumerate(grads, 1):
        _set_grads(ps, gs, has_grad=lambda i: has_grad(t, i))
        opt.step()
        if t < R.JOIN_FIRST:
            assert same_bits(ps[1].detach(), dev(p0[1])) and not bool(opt.state[ps[1]][0].any()) and not bool(opt.state[ps[1]][1].any())
        if t in R.JOIN_JUDGED:
            for i, p in enumerate(ps):
                judge3(fig, "step %d param %d" % (t, i), (p.detach(),) + tuple(opt.state[p]), r64[t - 1][i], t32[t - 1][i])
    fig.finish()
