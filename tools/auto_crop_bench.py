#!/usr/bin/env python3
"""What run_video(crop="auto") costs: host-to-host frames/s on a pinned-host 1280x720 uint8 clip (fp32 generator, ngf 64, 640x360
output) for crop=None, an explicit crop and crop="auto", at in_flight 1 and 2; one JSON line.  --kernel-only: 50 launches of
pws_field_homography on one 32-frame chunk of fields (run it under `rocprofv3 --kernel-trace --stats` for the kernel's time).
python tools/auto_crop_bench.py [--frames 256] [--kernel-only]"""
import argparse
import contextlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402
from pwstablenet_amd.lib.networks_cascading import define_G  # noqa: E402
from pwstablenet_amd.stream import VideoStabilizer, field_homography  # noqa: E402


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


def clip(T, H, W, seed=3):
    """A shaky clip: one smooth scene under small per-frame translations (synth.smooth_frames_u8), gray replicated to 3 channels."""
    base = synth.smooth_frames_u8(1, T, H, W, seed)[0]
    return torch.from_numpy(np.repeat(base[..., None], 3, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        xx = torch.linspace(-1, 1, 256, device="cuda")
        g = torch.stack(torch.meshgrid(xx, xx, indexing="xy"), -1)
        fields = torch.stack([g * (1.05 + 0.002 * i) + 0.01 for i in range(32)]).contiguous()
        for _ in range(50):
            field_homography(fields, (720, 1280))
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "launches": 50, "frames_per_launch": 32}))
        return
    with contextlib.redirect_stdout(sys.stderr):
        net = define_G(31, 2, 64, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=64)})
    net = net.cuda()
    T = a.frames
    u8_h = clip(T, 720, 1280).pin_memory()
    vs = VideoStabilizer(net, batch=32, swap_rb=True)
    rows = []
    for in_flight in (1, 2):
        row = {"in_flight": in_flight}
        run = lambda crop: vs.run_video(u8_h, chunk=32, half_size_output=True, crop=crop, in_flight=in_flight)   # noqa: E731
        row["none_fps"] = round(T / timed(lambda: run(None)), 1)
        try:
            t_auto = timed(lambda: run("auto"))
            row["auto_fps"] = round(T / t_auto, 1)
            window = tuple(round(v, 3) for v in vs_window(vs, u8_h))
        except ValueError as e:
            row["auto_error"] = str(e)[:200]
            window = (20.0, 620.0, 10.0, 350.0)
        row["window"] = window
        row["explicit_fps"] = round(T / timed(lambda: run(window)), 1)
        if "auto_fps" in row:
            row["auto_over_explicit"] = round(row["auto_fps"] / row["explicit_fps"], 3)
        rows.append(row)
    print(json.dumps({"frames": T, "source": "1280x720 uint8, pinned host", "output": "640x360 (half_size_output)", "math": "fp32",
                      "ngf": 64, "batch": 32, "chunk": 32, "rows": rows}))


def vs_window(vs, u8_h):
    """The window crop="auto" chose for this clip (fields recomputed as pass 1 forms them)."""
    from pwstablenet_amd.stream import auto_crop_window, window_planes
    T = u8_h.shape[0]
    planes = torch.cat([window_planes(u8_h[s:s + 32].cuda()) for s in range(0, T, 32)])
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    with torch.no_grad():
        for s in range(0, T, 32):
            e = min(T, s + 32)
            lo, hi = max(0, s - 15), min(T, e + 15)
            vs._fields(planes[lo:hi], s - lo, hi - e, fields[s:e])
    _, bounds = field_homography(fields, (720, 1280))
    return auto_crop_window(bounds, (720, 1280), (360, 640), vs.period)


if __name__ == "__main__":
    main()
