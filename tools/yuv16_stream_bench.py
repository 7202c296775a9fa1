#!/usr/bin/env python3
"""What the 10-bit 4:2:0 path costs, next to the 8-bit paths in the same process on the same box: (a) the fused 16-bit warp
(pws_upsample_grid_sample_yuv420_u16, P010 and I010) against the NV12 / I420 warp (pws_upsample_grid_sample_yuv420_u8) and the BGR byte warp
(pws_upsample_grid_sample_u8) on the same 8 stabiliser-like fields of 1280x720: us per launch from device events (tools/yuv_stream_bench.py's
method; the kernels alternate over several rounds, median and range reported), the ratio to NV12 and the fraction of 8 TB/s the algorithmic
frame traffic (6 / 3 / 6 bytes per pixel) reaches; (b) host-to-host frames/s of run_video(..., half_size_output=True) on a pinned-host
1280x720 clip as P010 and as NV12 (fp32 generator, ngf 64), in_flight 1 and 2.  The engine clock (rocm-smi, read right after the timed
loops) and the host's load average go into the result.  One JSON line, also written to --json.
python tools/yuv16_stream_bench.py [--frames 256] [--warp-only] [--json profiles/yuv16_stream_bench.json]"""
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


def launch_us(fn, iters=1000):
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
    """A shaky clip: one smooth scene under small per-frame translations (synth.smooth_frames_u8) with neutral chroma, as NV12 (Y rescaled
    to 16..235) and as P010 (the same Y at 10 bits, 64..940, word = v10 << 6)."""
    base = synth.smooth_frames_u8(1, T, H, W, seed)[0].astype(np.int32)
    nv12 = np.concatenate([(16 + base * 219 // 255).astype(np.uint8), np.full((T, H // 2, W), 128, np.uint8)], 1)
    p010 = np.concatenate([((64 + base * 876 // 255) << 6).astype(np.uint16), np.full((T, H // 2, W), 512 << 6, np.uint16)], 1)
    return torch.from_numpy(nv12), torch.from_numpy(p010)


def warp_rows(n=8, h=720, w=1280, rounds=5):
    xx = torch.linspace(-1, 1, 256, device="cuda")
    g = torch.stack(torch.meshgrid(xx, xx, indexing="xy"), -1)
    field = torch.stack([g * (1.02 + 0.002 * i) + 0.01 for i in range(n)]).contiguous()
    bgr = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
    yuv = torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8, device="cuda")
    y16 = torch.randint(0, 1024, (n, h * 3 // 2, w), dtype=torch.int32, device="cuda")
    src = {"p010": (y16 << 6).to(torch.uint16), "i010": y16.to(torch.uint16)}
    ob, oy, o16 = torch.empty_like(bgr), torch.empty_like(yuv), torch.empty_like(src["p010"])
    fns = {"bgr_u8": lambda: PF.upsample_grid_sample_u8(bgr, field, out=ob),
           "nv12": lambda: PF.upsample_grid_sample_yuv420(yuv, field, "nv12", out=oy),
           "i420": lambda: PF.upsample_grid_sample_yuv420(yuv, field, "i420", out=oy),
           "p010": lambda: PF.upsample_grid_sample_yuv420_16(src["p010"], field, "p010", out=o16),
           "i010": lambda: PF.upsample_grid_sample_yuv420_16(src["i010"], field, "i010", out=o16)}
    us = {k: [] for k in fns}
    for _ in range(rounds):   # the kernels alternate, so that a drift of clock or load hits all of them
        for k, fn in fns.items():
            us[k].append(launch_us(fn))
    bpp = {"bgr_u8": 6.0, "nv12": 3.0, "i420": 3.0, "p010": 6.0, "i010": 6.0}
    rows = {"launches_per_round": 1000, "rounds": rounds}
    med = {k: statistics.median(v) for k, v in us.items()}
    for k in fns:
        rows[k + "_us"] = round(med[k], 2)
        rows[k + "_us_range"] = [round(min(us[k]), 2), round(max(us[k]), 2)]
        rows[k + "_frac_8TBs"] = round(bpp[k] * n * h * w / (med[k] * 1e-6) / 8e12, 3)
    for k in ("p010", "i010"):
        rows[k + "_over_nv12"] = round(med[k] / med["nv12"], 3)
        rows[k + "_over_bgr"] = round(med[k] / med["bgr_u8"], 3)
    rows["i010_over_i420"] = round(med["i010"] / med["i420"], 3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warp-only", action="store_true")
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "yuv16_stream_bench.json"))
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
        nv12, p010 = clip(T, 720, 1280)
        nv12, p010 = nv12.pin_memory(), p010.pin_memory()
        vs = VideoStabilizer(net, batch=32)
        rows = []
        for in_flight in (1, 2):
            row = {"in_flight": in_flight}
            fps = {"nv12": [], "p010": []}
            for _ in range(2):   # alternating
                fps["nv12"].append(T / timed(lambda: vs.run_video(nv12, chunk=32, half_size_output=True, in_flight=in_flight, pixel_format="nv12")))
                fps["p010"].append(T / timed(lambda: vs.run_video(p010, chunk=32, half_size_output=True, in_flight=in_flight, pixel_format="p010")))
            row["nv12_fps"], row["p010_fps"] = round(max(fps["nv12"]), 1), round(max(fps["p010"]), 1)
            row["nv12_fps_all"], row["p010_fps_all"] = [round(v, 1) for v in fps["nv12"]], [round(v, 1) for v in fps["p010"]]
            row["p010_over_nv12"] = round(row["p010_fps"] / row["nv12_fps"], 3)
            # what PCIe moves per second at that rate: 1280 x 720 x 1.5 samples in, a quarter of that out, 2 bytes each
            row["p010_pcie_GBs_in_out"] = [round(row["p010_fps"] * 1280 * 720 * 3 / 1e9, 2), round(row["p010_fps"] * 640 * 360 * 3 / 1e9, 2)]
            rows.append(row)
        res["stream"] = {"frames": T, "source": "1280x720 pinned host", "output": "640x360 (half_size_output)", "math": "fp32", "ngf": 64,
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
