#!/usr/bin/env python3
"""What rigid warp mode costs.  (1) pws_field_rigid on 32 fields of 256 x 256 (16 MB in, 16 MB out) next to a device-to-device copy of the same
32 MB, in one process, alternating rounds, device events around `--launches` back-to-back launches per round; blended (r = 0.5) and fully
rigid (r = 1), with and without the statistics, out of place and in place.  (2) run_video host-to-host frames/s on a pinned-host 1280 x 720
uint8 clip (fp32 generator, ngf 64, 640 x 360 output) for rigidity 0 and rigidity 1 at in_flight 1 and 2, the two alternating inside every
round: the difference is the per-batch fit (one wave per frame, latency-bound) plus this kernel.  One JSON line; --json writes it to a file
as well.
python tools/rigid_bench.py [--frames 256] [--rounds 5] [--launches 200] [--kernel-only] [--json profiles/rigid_bench.json]"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pwstablenet_amd import functional as PF  # noqa: E402
from pwstablenet_amd import synth  # noqa: E402

FRAME = (720, 1280)


def events_ms(fn, launches):
    """device time of `launches` back-to-back calls of fn, per call, in ms"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def kernel_part(rounds, launches):
    from pwstablenet_amd.stream import field_homography
    n, fs = 32, 256
    xx = torch.linspace(-1, 1, fs, device="cuda")
    g = torch.stack(torch.meshgrid(xx, xx, indexing="xy"), -1)
    gen = torch.Generator(device="cuda").manual_seed(5)
    fields = torch.stack([g * (1.02 + 0.002 * i) + 0.01 for i in range(n)]).contiguous()
    fields += 0.01 * (torch.rand(fields.shape, device="cuda", generator=gen) - 0.5)   # (random data: not a field of trivial operands)
    m, bounds = field_homography(fields, FRAME)
    assert bool(torch.isfinite(bounds).all())
    out, dst, inplace = torch.empty_like(fields), torch.empty_like(fields), fields.clone()
    res = torch.empty((n,), device="cuda", dtype=torch.float32)
    unfit = torch.empty((n,), device="cuda", dtype=torch.int32)
    variants = {
        "copy_ms": lambda: dst.copy_(fields),
        "blend_ms": lambda: PF._field_rigid(fields, m, FRAME, 0.5, out, None, None),
        "rigid_ms": lambda: PF._field_rigid(fields, m, FRAME, 1.0, out, None, None),
        "rigid_stats_ms": lambda: PF._field_rigid(fields, m, FRAME, 1.0, out, res, unfit),
        "rigid_stats_in_place_ms": lambda: PF._field_rigid(inplace, m, FRAME, 1.0, inplace, res, unfit),
    }
    for fn in variants.values():   # warm-up: code objects, the allocator
        events_ms(fn, 10)
    samples = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            samples[name].append(events_ms(fn, launches))
    r = {"fields": "%d x %d x %d x 2 fp32" % (n, fs, fs), "bytes_moved": 2 * fields.numel() * 4, "rounds": rounds, "launches_per_round": launches}
    for name, v in samples.items():
        r[name] = {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
    for name in list(variants)[1:]:
        r[name[:-3] + "_over_copy"] = round(r[name]["median"] / r["copy_ms"]["median"], 3)
    r["rigid_stats_GBps"] = round(r["bytes_moved"] / r["rigid_stats_ms"]["median"] / 1e6, 1)
    r["residual_px_max"] = round(float(res.max()), 4)
    r["unfit_total"] = int(unfit.sum())
    return r


def stream_part(T, rounds):
    from pwstablenet_amd.lib.networks_cascading import define_G
    from pwstablenet_amd.stream import VideoStabilizer
    with contextlib.redirect_stdout(sys.stderr):
        net = define_G(31, 2, 64, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=64)})
    net = net.cuda()
    base = synth.smooth_frames_u8(1, T, FRAME[0], FRAME[1], 3)[0]
    u8_h = torch.from_numpy(np.repeat(base[..., None], 3, -1)).pin_memory()
    stabs = {"rigidity_0": VideoStabilizer(net, batch=32, swap_rb=True), "rigidity_1": VideoStabilizer(net, batch=32, swap_rb=True, rigidity=1.0)}
    rows = []
    for in_flight in (1, 2):
        times = {name: [] for name in stabs}
        row = {"in_flight": in_flight}

        def run(vs):
            vs.run_video(u8_h, chunk=32, half_size_output=True, in_flight=in_flight)
            torch.cuda.synchronize()
        for vs in stabs.values():   # warm-up of both paths
            run(vs)
        for _ in range(rounds):
            for name, vs in stabs.items():
                t0 = time.perf_counter()
                run(vs)
                times[name].append(time.perf_counter() - t0)
        for name, v in times.items():
            row[name + "_fps"] = {"median": round(T / statistics.median(v), 1), "min": round(T / max(v), 1), "max": round(T / min(v), 1)}
        row["rigidity_1_over_0"] = round(row["rigidity_1_fps"]["median"] / row["rigidity_0_fps"]["median"], 3)
        row["residual_px_max"] = round(float(stabs["rigidity_1"].rigid_residual.max()), 3)
        row["unfit_total"] = int(stabs["rigidity_1"].rigid_unfit.sum())
        rows.append(row)
    return {"frames": T, "source": "1280x720 uint8, pinned host", "output": "640x360 (half_size_output)", "math": "fp32", "ngf": 64, "batch": 32,
            "chunk": 32, "rounds": rounds, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--json", metavar="PATH", help="also write the result, indented, to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rigid_bench: no GPU visible (timings are taken on the device only)")
    res = {"kernel": kernel_part(a.rounds, a.launches)}
    if not a.kernel_only:
        res["run_video"] = stream_part(a.frames, a.rounds)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
