#!/usr/bin/env python3
"""What the 4:2:0 YUV path costs: (1) the fused YUV warp (pws_upsample_grid_sample_yuv420_u8, NV12 and I420) against the BGR byte warp
(pws_upsample_grid_sample_u8) on the same 8 fields of 1280x720, us per launch from device events and the fraction of 8 TB/s their
algorithmic frame traffic (3 / 6 bytes per pixel) reaches; (2) host-to-host frames/s of run_video(..., half_size_output=True) on a
pinned-host 1280x720 clip as NV12 and as BGR (fp32 generator, ngf 64), in_flight 1 and 2.  One JSON line.
python tools/yuv_stream_bench.py [--frames 256] [--warp-only]"""
import argparse
import contextlib
import json
import os
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


def launch_us(fn, iters=200):
    for _ in range(20):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def clip(T, H, W, seed=3):
    """A shaky clip: one smooth scene under small per-frame translations (synth.smooth_frames_u8): gray as BGR, and as NV12 with
    neutral chroma (the same Y rescaled to 16..235)."""
    base = synth.smooth_frames_u8(1, T, H, W, seed)[0]
    bgr = np.repeat(base[..., None], 3, -1)
    nv12 = np.concatenate([(16 + base.astype(np.int32) * 219 // 255).astype(np.uint8), np.full((T, H // 2, W), 128, np.uint8)], 1)
    return torch.from_numpy(bgr), torch.from_numpy(nv12)


def warp_rows(n=8, h=720, w=1280):
    xx = torch.linspace(-1, 1, 256, device="cuda")
    g = torch.stack(torch.meshgrid(xx, xx, indexing="xy"), -1)
    field = torch.stack([g * (1.02 + 0.002 * i) + 0.01 for i in range(n)]).contiguous()
    bgr = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
    yuv = torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8, device="cuda")
    ob, oy = torch.empty_like(bgr), torch.empty_like(yuv)
    rows = {}
    t_bgr = launch_us(lambda: PF.upsample_grid_sample_u8(bgr, field, out=ob))
    rows["bgr_u8_us"] = round(t_bgr, 2)
    rows["bgr_u8_frac_8TBs"] = round(6.0 * n * h * w / (t_bgr * 1e-6) / 8e12, 3)
    for fmt in ("nv12", "i420"):
        t = launch_us(lambda: PF.upsample_grid_sample_yuv420(yuv, field, fmt, out=oy))
        rows[fmt + "_us"] = round(t, 2)
        rows[fmt + "_over_bgr"] = round(t / t_bgr, 3)
        rows[fmt + "_frac_8TBs"] = round(3.0 * n * h * w / (t * 1e-6) / 8e12, 3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warp-only", action="store_true")
    a = ap.parse_args()
    res = {"warp": dict(frames=8, size="1280x720", **warp_rows())}
    if not a.warp_only:
        from pwstablenet_amd.lib.networks_cascading import define_G
        from pwstablenet_amd.stream import VideoStabilizer
        with contextlib.redirect_stdout(sys.stderr):
            net = define_G(31, 2, 64, "normal", 0.02)
        net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=64)})
        net = net.cuda()
        T = a.frames
        bgr, nv12 = clip(T, 720, 1280)
        bgr, nv12 = bgr.pin_memory(), nv12.pin_memory()
        vs = VideoStabilizer(net, batch=32, swap_rb=True)
        rows = []
        for in_flight in (1, 2):
            row = {"in_flight": in_flight}
            row["bgr_fps"] = round(T / timed(lambda: vs.run_video(bgr, chunk=32, half_size_output=True, in_flight=in_flight)), 1)
            row["nv12_fps"] = round(T / timed(lambda: vs.run_video(nv12, chunk=32, half_size_output=True, in_flight=in_flight,
                                                                   pixel_format="nv12")), 1)
            row["nv12_over_bgr"] = round(row["nv12_fps"] / row["bgr_fps"], 3)
            rows.append(row)
        res["stream"] = {"frames": T, "source": "1280x720 pinned host", "output": "640x360 (half_size_output)", "math": "fp32", "ngf": 64,
                         "batch": 32, "chunk": 32, "rows": rows}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
