#!/usr/bin/env python3
"""Identity A/B of the field-domain kernels (csrc/field_zoom.hip, field_compose.hip, field_rigid.hip, field_wobble.hip, field_reach.hip)
across a refactor: the six C entries on small seeded inputs with two builds of the package, per case the SHA-256 of every output and of
every statistics buffer (pre-filled with 0x7f bytes, so the entry's clear is part of what is compared).  Every hash must be equal.

One build per process, each under its own time limit; the second checkout holds the other commit, built:

    timeout -k 10 300 python tools/field_ab.py --root ../parent --json profiles/field_lattice_ab_parent.json && \\
    timeout -k 10 300 python tools/field_ab.py --json profiles/field_lattice_ab_head.json && \\
    python tools/field_ab.py --compare profiles/field_lattice_ab_parent.json profiles/field_lattice_ab_head.json

Cases: all six entries on tests/zoom_ref.py's SHAPES (256 x 256, 24 x 40, 2 x 2 and the odd-width 67 x 129), statistics given and NULL, a NaN
and an infinity in the field, a frame whose homography is NaN; pws_field_rigid in place and at rigidity 0, 0.5, 1; pws_field_compose_rows at
r = 0 and 0.8 with zero and non-zero rates; pws_field_wobble on 1, 33 and 70 frames of 24 x 40 (both sides of a 32-frame segment) at sigma 1/3
and 5 (R = 1 and 15); pws_field_reach on rectangles of 67 x 129 whose origin and extent are no multiples of 4 rows / 128 columns, on one
node, at levels 0 and 64, with rates and without.

--bench: the kernel figures (not the streaming legs) of tools/zoom_bench.py, rigid_bench.py, path_smooth_bench.py, rolling_shutter_bench.py,
wobble_bench.py and path_limit_bench.py of the checkout --root, one process per run; --window PARENT.json HEAD.json applies
profiles/README.md's rule to the runs that each file has collected (--json appends a run)."""
import argparse
import hashlib
import json
import os
import sys

FRAME = (360, 640)
SHAPES = [(3, 256, 256, 2), (2, 24, 40, 2), (1, 2, 2, 2), (5, 67, 129, 2)]   # tests/zoom_ref.py SHAPES


def sha(t):
    import torch
    t = t.detach().to("cpu").contiguous().reshape(-1)
    return "%s:%d:%s" % (str(t.dtype)[6:], t.numel(), hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest())


def inputs(shape, seed):
    """field with a NaN and an infinity, coef, d (frame 0: the identity), rates, m (the last frame's: NaN, when there are two), on the device"""
    import numpy as np
    import torch
    T, fh, fw, _ = shape
    rs = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(np.linspace(-1, 1, fw), np.linspace(-1, 1, fh), indexing="xy"), -1)
    field = (1.04 * g[None] + 0.03 * rs.normal(size=shape)).astype(np.float32)
    field[0, 1, 1, 0], field[T - 1, fh - 1, 0, 1] = np.nan, np.inf
    coef = np.stack([3 * rs.rand(T), 0.9 + 0.1 * rs.rand(T), 2 * rs.rand(T), 0.9 + 0.1 * rs.rand(T)], 1).astype(np.float32)
    th, sc = np.deg2rad(rs.normal(0, 0.5, T)), np.exp(rs.normal(0, 0.02, T))
    d = np.stack([sc * np.cos(th), -sc * np.sin(th), rs.normal(0, 9, T), sc * np.sin(th), sc * np.cos(th), rs.normal(0, 6, T)], 1)
    d[0] = [1, 0, 0, 0, 1, 0]
    coef[0] = [0, 1, 0, 1]
    rates = rs.normal(0, 1, (T, 2, 4)) * np.array([0.004, 0.002, 6.0, 4.0])
    m = np.tile(np.eye(3).reshape(1, 9), (T, 1)) + rs.normal(0, 0.01, (T, 9)) * np.array([1, 1, 1, 1, 1, 1, 0.3, 0.3, 0])
    if T > 1:
        m[T - 1, 4] = np.nan
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (field, coef, d, rates, m)]


def run_cases():
    import torch
    from pwstablenet_amd import hipabi as A
    L, out = A.lib(), {}
    h0, w0 = FRAME

    def junk(shape, dtype):
        return torch.full(shape, 0x7f7f7f7f, dtype=torch.int32, device="cuda").view(dtype)

    def put(name, entry, rc, *tensors):
        A.check(rc, entry)
        torch.cuda.synchronize()
        out[name] = [sha(t) for t in tensors if t is not None]
        print(name, out[name][0][-16:], flush=True)

    def wobble(tag, field, m, sigmas):
        n, fh, fw, _ = field.shape
        for sigma in sigmas:
            for stats in (True, False):
                o = junk(field.shape, torch.float32)
                s0, s1 = (junk((n,), torch.float32), junk((n,), torch.int32)) if stats else (None, None)
                put("wobble %s sigma %.3f stats %d" % (tag, sigma, stats), "pws_field_wobble",
                    L.pws_field_wobble(A.ptr(field), n, fh, fw, A.ptr(m), sigma, h0, w0, A.ptr(o), A.ptr(s0), A.ptr(s1), A.current_stream()), o, s0, s1)

    def reach(tag, field, d, rates, levels, rect, r, margin=0):
        n, fh, fw, _ = field.shape
        lam = torch.linspace(0, 1, levels + 1, dtype=torch.float64, device="cuda")[None, :, None] if levels else torch.ones((1, 1, 1), dtype=torch.float64, device="cuda")
        eye = torch.tensor([1.0, 0, 0, 0, 1, 0], dtype=torch.float64, device="cuda")
        table = (eye + lam * (d[:, None, :] - eye)).contiguous()
        counts = junk((n, levels + 1), torch.int32)
        put("reach %s levels %d rect %s r %.1f margin %d" % (tag, levels, "-".join(map(str, rect)), r, margin), "pws_field_reach",
            L.pws_field_reach(A.ptr(field), n, fh, fw, A.ptr(table), levels, A.ptr(rates) if r else None, r, rect[0], rect[1], rect[2], rect[3], h0, w0,
                              0, margin, A.ptr(counts), A.current_stream()), counts)

    for shape in SHAPES:
        n, fh, fw, _ = shape
        tag = "%dx%dx%d" % shape[:3]
        field, coef, d, rates, m = inputs(shape, 11 + fw)
        zero_rates = torch.zeros_like(rates)
        for stats in (True, False):
            for ac, margin in ((0, 0), (1, 1)):
                o, unc = junk(shape, torch.float32), junk((n,), torch.int32) if stats else None
                put("zoom %s stats %d ac %d margin %d" % (tag, stats, ac, margin), "pws_field_zoom",
                    L.pws_field_zoom(A.ptr(field), n, fh, fw, A.ptr(coef), A.ptr(o), h0, w0, ac, margin, A.ptr(unc), A.current_stream()), o, unc)
                o, unc = junk(shape, torch.float32), junk((n,), torch.int32) if stats else None
                put("compose %s stats %d ac %d margin %d" % (tag, stats, ac, margin), "pws_field_compose",
                    L.pws_field_compose(A.ptr(field), n, fh, fw, A.ptr(d), A.ptr(o), h0, w0, ac, margin, A.ptr(unc), A.current_stream()), o, unc)
            for r in (0.0, 0.8):
                for rt, rname in ((zero_rates, "zero"), (rates, "rates")):
                    o, unc = junk(shape, torch.float32), junk((n,), torch.int32) if stats else None
                    put("compose_rows %s stats %d r %.1f %s" % (tag, stats, r, rname), "pws_field_compose_rows",
                        L.pws_field_compose_rows(A.ptr(field), n, fh, fw, A.ptr(d), A.ptr(rt), r, A.ptr(o), h0, w0, 0, 0, A.ptr(unc),
                                                 A.current_stream()), o, unc)
            for rigidity in (0.0, 0.5, 1.0):
                for in_place in (False, True):
                    src = field.clone()
                    o = src if in_place else junk(shape, torch.float32)
                    s0, s1 = (junk((n,), torch.float32), junk((n,), torch.int32)) if stats else (None, None)
                    put("rigid %s stats %d rigidity %.1f in_place %d" % (tag, stats, rigidity, in_place), "pws_field_rigid",
                        L.pws_field_rigid(A.ptr(src), n, fh, fw, A.ptr(m), rigidity, h0, w0, A.ptr(o), A.ptr(s0), A.ptr(s1), A.current_stream()),
                        o, s0, s1)
        wobble(tag, field, m, (1.0 / 3, 5.0))
        reach(tag, field, d, rates, 4, (0, fh - 1, 0, fw - 1), 0.0)
        reach(tag, field, d, rates, 4, (0, fh - 1, 0, fw - 1), 0.8, margin=1)
    for n in (1, 33, 70):   # both sides of a 32-frame segment
        field, _, _, _, m = inputs((n, 24, 40, 2), 100 + n)
        wobble("%dx24x40" % n, field, m, (1.0 / 3, 5.0))
    field, _, d, rates, _ = inputs((5, 67, 129, 2), 7)
    for rect in ((3, 65, 1, 128), (0, 66, 0, 128), (5, 9, 127, 128), (10, 10, 77, 77), (66, 66, 128, 128)):
        for levels in (0, 64):
            for r in (0.0, 0.8):
                reach("5x67x129", field, d, rates, levels, rect, r)
    return out


def bench(root):
    """The kernel figures of the six tools of ``root``: {tool: its own rows}."""
    sys.argv += ["--package-root", root]   # (four of the tools read it at import)
    sys.path.insert(0, os.path.join(root, "tools"))
    import path_limit_bench
    import path_smooth_bench
    import rigid_bench
    import rolling_shutter_bench
    import wobble_bench
    import zoom_bench
    return {"zoom_bench": zoom_bench.kernel_part(5, 200), "rigid_bench": rigid_bench.kernel_part(5, 200),
            "path_smooth_bench": path_smooth_bench.kernel_rows(), "rolling_shutter_bench": rolling_shutter_bench.kernel_rows(),
            "wobble_bench": wobble_bench.kernel_rows(), "path_limit_bench": path_limit_bench.kernel_rows()}


def figures(run):
    """{figure: (a run's best, its worst), in microseconds} of one bench() result."""
    out = {}
    for tool, rows in run.items():
        for k, v in rows.items():
            if k.endswith("_us_range"):
                out["%s %s" % (tool, k[:-9])] = (v[0], v[1])
            elif isinstance(v, dict) and "min" in v:   # (the two older tools write milliseconds)
                out["%s %s" % (tool, k[:-3])] = (round(v["min"] * 1e3, 2), round(v["max"] * 1e3, 2))
    return out


def window(parent, head):
    """The rule of profiles/README.md: a head figure (a run's best) passes if it is not above the parent's highest best-of-run plus the
    parent's own spread between repeats.  Prints a table row per figure; returns the figures outside."""
    with open(parent) as f:
        p = [figures(r) for r in json.load(f)["runs"]]
    with open(head) as f:
        h = [figures(r) for r in json.load(f)["runs"]]
    outside = []
    print("| figure (us) | parent's bests | spread | limit | head's bests | |\n|---|---|---|---|---|---|")
    for k in sorted(p[0]):
        bests, spread = [r[k][0] for r in p], max(r[k][1] - r[k][0] for r in p)
        limit = max(bests) + spread
        heads = [r[k][0] for r in h]
        bad = [v for v in heads if v > limit + 1e-9]
        outside += [k] * bool(bad)
        print("| %s | %s | %.2f | %.2f | %s | %s |" % (k, ", ".join("%.2f" % v for v in bests), spread, limit, ", ".join("%.2f" % v for v in heads),
                                                     "OUTSIDE" if bad else "inside"))
    return outside


def compare(a, b):
    with open(a) as f:
        x = json.load(f)["cases"]
    with open(b) as f:
        y = json.load(f)["cases"]
    bad = [k for k in sorted(set(x) | set(y)) if x.get(k) != y.get(k)]
    print("\n".join("%s differs" % k for k in bad) if bad else "identical: %d cases, %d hashes" % (len(x), sum(len(v) for v in x.values())))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package runs")
    ap.add_argument("--json")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--window", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if args.window:
        sys.exit(1 if window(*args.window) else 0)
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import pwstablenet_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(pwstablenet_amd.__file__))) == root, pwstablenet_amd.__file__
    if args.bench:
        runs = []
        if os.path.exists(args.json):
            with open(args.json) as f:
                runs = json.load(f)["runs"]
        runs.append(bench(root))
        with open(args.json, "w") as f:
            json.dump({"runs": runs}, f, indent=1, sort_keys=True)
        return
    cases = run_cases()
    with open(args.json, "w") as f:   # (a case a line)
        f.write('{"cases": {\n%s\n}}\n' % ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(cases.items())))


if __name__ == "__main__":
    main()
