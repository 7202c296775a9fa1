#!/usr/bin/env python3
"""What bicubic interpolation costs next to bilinear, in one process on the same box: (a) every fused warp (fp32 NCHW, BGR bytes, NV12 / I420,
P010 / I010) with mode="bilinear" and mode="bicubic" on the same 8 stabiliser-like fields of 1280x720: us per launch from device events
(tools/yuv16_stream_bench.py's method; the kernels alternate over several rounds, median and range reported) and the ratio bicubic / bilinear;
(b) host-to-host frames/s of run_video on a pinned-host 1280x720 clip at full output size, as BGR and as NV12, with both interpolations, at
in_flight 1 and 2 (fp32 generator, ngf 64).  The engine clock (rocm-smi, read right after the timed loops) and the host's load average go into
the result.  One JSON line, also written to --json.
python tools/bicubic_warp_bench.py [--frames 128] [--warp-only] [--json profiles/bicubic_warp_bench.json]"""
import argparse
import contextlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pwstablenet_amd import functional as PF  # noqa: E402
from pwstablenet_amd import synth  # noqa: E402

MODES = ("bilinear", "bicubic")


def timed(fn, reps=2):
    fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def launch_us(fn, iters=500):
    for _ in range(20):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def engine_clock():
    """sclk as `rocm-smi --showclocks` reports it, or None.  A read-only query: this tool never sets or resets anything on the device, and
    must not grow a flag that does."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        m = re.search(r"sclk[^\n]*?\((\d+)\s*Mhz\)", out, re.I)
        return int(m.group(1)) if m else None
    except (OSError, subprocess.SubprocessError):
        return None


def clip(T, H, W, seed=3):
    """A shaky clip: one smooth scene under small per-frame translations (synth.smooth_frames_u8), as BGR (the scene in every channel) and as
    NV12 (Y rescaled to 16..235, neutral chroma)."""
    base = synth.smooth_frames_u8(1, T, H, W, seed)[0]
    bgr = np.ascontiguousarray(np.repeat(base[..., None], 3, -1))
    nv12 = np.concatenate([(16 + base.astype(np.int32) * 219 // 255).astype(np.uint8), np.full((T, H // 2, W), 128, np.uint8)], 1)
    return torch.from_numpy(bgr), torch.from_numpy(nv12)


def warp_rows(n=8, h=720, w=1280, rounds=3):
    xx = torch.linspace(-1, 1, 256, device="cuda")
    g = torch.stack(torch.meshgrid(xx, xx, indexing="xy"), -1)
    field = torch.stack([g * (1.02 + 0.002 * i) + 0.01 for i in range(n)]).contiguous()
    f32 = torch.rand((n, 3, h, w), device="cuda") * 255
    bgr = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
    yuv = torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8, device="cuda")
    y16 = torch.randint(0, 1024, (n, h * 3 // 2, w), dtype=torch.int32, device="cuda")
    src = {"p010": (y16 << 6).to(torch.uint16), "i010": y16.to(torch.uint16)}
    ob, oy, o16 = torch.empty_like(bgr), torch.empty_like(yuv), torch.empty_like(src["p010"])
    fns = {}
    for m in MODES:
        fns["fp32", m] = lambda m=m: PF.upsample_grid_sample(f32, field, mode=m)
        fns["bgr_u8", m] = lambda m=m: PF.upsample_grid_sample_u8(bgr, field, out=ob, mode=m)
        for fmt in ("nv12", "i420"):
            fns[fmt, m] = lambda m=m, fmt=fmt: PF.upsample_grid_sample_yuv420(yuv, field, fmt, out=oy, mode=m)
        for fmt in ("p010", "i010"):
            fns[fmt, m] = lambda m=m, fmt=fmt: PF.upsample_grid_sample_yuv420_16(src[fmt], field, fmt, out=o16, mode=m)
    us = {k: [] for k in fns}
    for _ in range(rounds):   # the kernels alternate, so that a drift of clock or load hits all of them
        for k, fn in fns.items():
            us[k].append(launch_us(fn))
    rows = {"launches_per_round": 500, "rounds": rounds}
    med = {k: statistics.median(v) for k, v in us.items()}
    for (fmt, m), v in med.items():
        rows["%s_%s_us" % (fmt, m)] = round(v, 2)
        rows["%s_%s_us_range" % (fmt, m)] = [round(min(us[fmt, m]), 2), round(max(us[fmt, m]), 2)]
    for fmt in ("fp32", "bgr_u8", "nv12", "i420", "p010", "i010"):
        rows[fmt + "_bicubic_over_bilinear"] = round(med[fmt, "bicubic"] / med[fmt, "bilinear"], 3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--warp-only", action="store_true")
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bicubic_warp_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "load_avg_before": [round(v, 1) for v in os.getloadavg()]}
    res["warp"] = dict(frames=8, size="1280x720", **warp_rows())
    res["sclk_mhz_after_warp_loops"] = engine_clock()
    if not a.warp_only:
        from pwstablenet_amd.lib.networks_cascading import define_G
        from pwstablenet_amd.stream import VideoStabilizer
        with contextlib.redirect_stdout(sys.stderr):
            net = define_G(31, 2, 64, "normal", 0.02)
        net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=64)})
        net = net.cuda()
        T = a.frames
        clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in clip(T, 720, 1280))))
        vs = {m: VideoStabilizer(net, batch=32, interpolation=m) for m in MODES}
        rows = []
        for in_flight in (1, 2):
            row = {"in_flight": in_flight}
            fps = {(fmt, m): [] for fmt in clips for m in MODES}
            for _ in range(2):   # alternating
                for (fmt, m), v in fps.items():
                    v.append(T / timed(lambda: vs[m].run_video(clips[fmt], chunk=32, in_flight=in_flight, pixel_format=fmt)))
            for (fmt, m), v in fps.items():
                row["%s_%s_fps" % (fmt, m)] = round(max(v), 1)
                row["%s_%s_fps_all" % (fmt, m)] = [round(x, 1) for x in v]
            for fmt in clips:
                row[fmt + "_bicubic_over_bilinear"] = round(row[fmt + "_bicubic_fps"] / row[fmt + "_bilinear_fps"], 3)
            rows.append(row)
        res["stream"] = {"frames": T, "source": "1280x720 pinned host", "output": "1280x720 (full size)", "math": "fp32", "ngf": 64,
                         "batch": 32, "chunk": 32, "rows": rows}
        res["sclk_mhz_after_stream"] = engine_clock()
    res["load_avg_after"] = [round(v, 1) for v in os.getloadavg()]
    line = json.dumps(res)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
