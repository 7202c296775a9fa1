"""Float64 Adam, the torch-fp32 yardstick and the inputs of tests/test_hip_adam_float64.py (GPU) and tests/test_adam_ref64_cpu.py (no GPU):
both files draw their cases from the builders here, so the CPU test can show that the rule is attainable, and that it has teeth, on
exactly the numbers the kernels are later given.

  step      the truth: float64 numpy, torch's formulation, the hyper-parameters as the Python doubles the caller wrote
  torch32   the yardstick: one step of torch.optim.Adam(foreach=False) in fp32 on the CPU from a given state
  kernel32  csrc/adam.hip restated in numpy fp32 (adam_update's fused multiply-adds included), with the complements 1 - beta formed either in double on the
            host (the fixed arithmetic) or as 1.f - (float)beta (what the kernels did before)

All three take (p, g, m, v, lr, beta1, beta2, eps, step), leave their arguments alone and return new (p, m, v)."""
import os
import re

import numpy as np

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (lr, beta1, beta2, eps): the reference's (main_new.py:63), the common default betas, bench.py's, a coarse one
HYPERS = [(1e-3, 0.5, 0.999, 1e-8), (1e-4, 0.9, 0.999, 1e-8), (1e-6, 0.5, 0.999, 1e-8), (1e-2, 0.9, 0.99, 1e-6)]
STEPS = [1, 2, 3, 10, 1000, 100000]
# magnitude classes of (a): sqrt(v) far below, at and far above eps; g^2 from 1e-30 to 1e30, all normal fp32 numbers
SCALES = [1e-15, 1e-8, 1e-4, 1.0, 1e4, 1e15]
SUBNORMAL_SCALE = 1e-20          # (d): g^2 ~ 1e-40, below 2^-126
N_CLASS = 4099                   # one full workgroup of the multi kernel (4096) + a ragged scalar tail of 3
TINY32 = 2.0 ** -126             # the smallest normal fp32 number

RUN_STEPS, RUN_JUDGED, RUN_N = 50, (1, 2, 10, 50), 4099          # (b)
GRID_STRIDE_COUNT = 2048 * 256 * 4 + 1024 + 3                      # (e)
TABLE_PATTERN = [1, 3, 4, 4095, 4096, 4097, 8192, 8193]            # (f)
TABLE_EMPTY = (0, 47, 48, 99)
CLASS_NUMELS = [1, 63, 64, 65, 4097, 3 * 5 * 7, 512 * 16, 2, 100003]   # (h)
CLASS_SHAPES = [(1,), (63,), (64,), (5, 13), (4097,), (3, 5, 7), (512, 16), (2,), (100003,)]
CLASS_STEPS, CLASS_JUDGED, CLASS_TRANSPOSED = 12, (1, 2, 12), 6    # parameter 6 gets its gradients as transposed views
JOIN_STEPS, JOIN_FIRST, JOIN_JUDGED = 6, 4, (4, 6)                  # (i)


# ------------------------------------------------------------------------------------------------------------ the three Adams
def step(p, g, m, v, lr, beta1, beta2, eps, step):
    """float64, torch's formulation; nothing is ever rounded to fp32"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    with np.errstate(invalid="ignore", over="ignore"):
        p = p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return p, m, v


def torch32(p, g, m, v, lr, beta1, beta2, eps, step):
    """one step of torch.optim.Adam(foreach=False), fp32, CPU, from the state (step - 1, m, v)"""
    import torch
    t = torch.from_numpy(np.array(p, dtype=F32)).requires_grad_(True)
    opt = torch.optim.Adam([t], lr=lr, betas=(beta1, beta2), eps=eps, foreach=False)
    opt.state[t] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(np.array(m, dtype=F32)),
                    "exp_avg_sq": torch.from_numpy(np.array(v, dtype=F32))}
    t.grad = torch.from_numpy(np.array(g, dtype=F32))
    opt.step()
    st = opt.state[t]
    assert float(st["step"]) == step
    return t.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def kernel32(p, g, m, v, lr, beta1, beta2, eps, step, complement="host"):
    """adam_kernel / adam_multi_kernel and their host side, operation by operation in fp32.  complement: "host" = (float)(1.0 - beta)
    from the doubles (pws_adam_step_d), "device" = 1.f - (float)beta (the kernels before)."""
    p, g, m, v = (np.array(a, dtype=F32) for a in (p, g, m, v))
    b1, b2, e = F32(beta1), F32(beta2), F32(eps)
    c1, c2 = (F32(1.0 - beta1), F32(1.0 - beta2)) if complement == "host" else (F32(1) - b1, F32(1) - b2)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    step_size, inv_bc2_sqrt = F32(lr / bc1), F32(1.0 / np.sqrt(bc2))
    # a fused multiply-add: the product of two fp32 numbers is exact in float64, the sum is rounded there and once more to fp32
    fma = lambda a, b, c: (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)  # noqa: E731
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        m = fma(b1, m, c1 * g)
        v = fma(c2 * g, g, b2 * v)
        p = fma(-step_size, m / fma(np.sqrt(v), inv_bc2_sqrt, e), p)
    assert p.dtype == m.dtype == v.dtype == F32
    return p, m, v


# ------------------------------------------------------------------------------------------------------------ builders
def moment_case(n, scale, seed, state="given", p0="zero"):
    """fp32 (p, g, m, v) of one magnitude class: m ~ 0.1 N(0,1) s, v ~ U(0,1) s^2, g ~ N(0,1) s; state="zero": m = v = 0 (the first
    step).  p0: "zero" (the judged p is the displacement) or "normal" (N(0,1), for comparisons of bits only)."""
    rs = np.random.RandomState(seed)
    g = (rs.standard_normal(n) * scale).astype(F32)
    m = (0.1 * rs.standard_normal(n) * scale).astype(F32)
    v = (rs.uniform(0, 1, n) * scale * scale).astype(F32)
    p = rs.standard_normal(n).astype(F32)
    if state == "zero":
        m[:], v[:] = 0, 0
    if p0 == "zero":
        p[:] = 0
    return {"p": p, "g": g, "m": m, "v": v, "scale": scale}


def one_step_classes(state="given"):
    """(a): one moment_case of N_CLASS elements per magnitude class.  From zero moments v is (1 - beta2) g^2 alone, sub-normal for the
    smaller g of the class s = 1e-15 (that is (d)'s subject): the zero state runs without that class."""
    return [moment_case(N_CLASS, s, 100 + i, state) for i, s in enumerate(SCALES) if state == "given" or i > 0]


def run_gradients(n=RUN_N, steps=RUN_STEPS, seed=7):
    """(b): fp32 gradients of `steps` consecutive steps, each N(0,1) times a scale drawn log-uniformly from four decades"""
    rs = np.random.RandomState(seed)
    return [(rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 1)).astype(F32) for _ in range(steps)]


def table_counts():
    """(f): 100 counts, TABLE_PATTERN repeated, zero at TABLE_EMPTY"""
    return [0 if i in TABLE_EMPTY else TABLE_PATTERN[i % len(TABLE_PATTERN)] for i in range(100)]


def table_case(seed=11):
    """(f): one moment_case (scale 1) over all the table's elements, and the offsets that cut it into the 100 tensors"""
    counts = table_counts()
    c = moment_case(sum(counts), 1.0, seed)
    c["counts"], c["offsets"] = counts, np.concatenate([[0], np.cumsum(counts)]).tolist()
    return c


def class_case(seed=13, lr=1e-3):
    """(h): initial parameters of CLASS_SHAPES, |p0| <= 1e-3 lr, and CLASS_STEPS gradients per parameter (one scale per step)"""
    rs = np.random.RandomState(seed)
    p0 = [(rs.uniform(-1, 1, s) * 1e-3 * lr).astype(F32) for s in CLASS_SHAPES]
    grads = []
    for _ in range(CLASS_STEPS):
        scale = 10.0 ** rs.uniform(-3, 1)
        grads.append([(rs.standard_normal(s) * scale).astype(F32) for s in CLASS_SHAPES])
    return p0, grads


def join_case(seed=17):
    """(i): three parameters and JOIN_STEPS gradients each.  0 has a gradient in every step; 1 from step JOIN_FIRST on; 2 is made after the
    optimiser and has a gradient in every step."""
    rs = np.random.RandomState(seed)
    shapes = [(70,), (4099,), (5, 13)]
    p0 = [np.zeros(s, F32) for s in shapes]
    grads = [[rs.standard_normal(s).astype(F32) for s in shapes] for _ in range(JOIN_STEPS)]
    has_grad = lambda t, i: i != 1 or t >= JOIN_FIRST  # noqa: E731  (t counts from 1)
    return p0, grads, has_grad


def run64(p0, grads, hyper, has_grad=lambda t, i: True):
    """float64 Adam with torch's per-parameter step over lists of parameters: [(p, m, v) per parameter] after every step"""
    st = [[np.asarray(p, np.float64), np.zeros(p.shape), np.zeros(p.shape), 0] for p in p0]
    out = []
    for t, gs in enumerate(grads, 1):
        for i, g in enumerate(gs):
            if has_grad(t, i):
                st[i][3] += 1
                st[i][0], st[i][1], st[i][2] = step(st[i][0], g, st[i][1], st[i][2], *hyper, st[i][3])
        out.append([(s[0], s[1], s[2]) for s in st])
    return out


def run_torch32(p0, grads, hyper, has_grad=lambda t, i: True):
    """the same with one torch.optim.Adam(foreach=False), fp32, CPU, over all the parameters: [(p, m, v) or (p, None, None)] per step"""
    import torch
    ps = [torch.from_numpy(np.array(p, dtype=F32)).requires_grad_(True) for p in p0]
    lr, b1, b2, eps = hyper
    opt = torch.optim.Adam(ps, lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    out = []
    for t, gs in enumerate(grads, 1):
        for i, (p, g) in enumerate(zip(ps, gs)):
            p.grad = torch.from_numpy(g.copy()) if has_grad(t, i) else None
        opt.step()
        out.append([(p.detach().numpy().copy(),) + ((opt.state[p]["exp_avg"].numpy().copy(), opt.state[p]["exp_avg_sq"].numpy().copy())
                                                     if p in opt.state and len(opt.state[p]) else (None, None)) for p in ps])
    return out


# ------------------------------------------------------------------------------------------------------------ the sources' constants
def kernel_constants():
    """What the cases are sized against, read from the text of csrc/adam.hip"""
    src = open(os.path.join(ROOT, "pwstablenet_amd", "csrc", "adam.hip")).read()
    grab = lambda pat: int(re.search(pat, src).group(1))  # noqa: E731
    return {"max_tensors": grab(r"constexpr int kAdamMaxTensors = (\d+);"), "grid_cap": grab(r"if \(blocks > (\d+)\) blocks = \1;"),
            "lanes": grab(r"__launch_bounds__\((\d+)\) adam_kernel"), "block_elems": grab(r"\(blockIdx\.x - a\.first_block\[lo\]\) \* (\d+);"),
            "unaligned_max": grab(r"PWS_REQUIRE\(count <= (\d+), \"pws_adam_step: buffers must be 16-byte aligned")}


def table_launches(counts, max_tensors):
    """the host loop of pws_adam_step_multi_d: [(indices of one launch's tensors)], and the passes that end with nothing to launch"""
    launches, empty, i = [], 0, 0
    while i < len(counts):
        cur = []
        while i < len(counts) and len(cur) < max_tensors:
            if counts[i]:
                cur.append(i)
            i += 1
        if cur:
            launches.append(cur)
        else:
            empty += 1
    return launches, empty
