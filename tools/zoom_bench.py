#!/usr/bin/env python3
"""What zoom to fill costs.  (1) pws_field_zoom on 32 fields of 256 x 256 (16 MB in, 16 MB out) next to a device-to-device copy of the same
32 MB, in one process, alternating rounds, device events around `--launches` back-to-back launches per round; with and without the
uncovered count.  (2) run_video host-to-host frames/s on a pinned-host 1280 x 720 uint8 clip (fp32 generator, ngf 64, 640 x 360 output) for
zoom=None, zoom="auto" and crop="auto" at in_flight 1 and 2, the three alternating inside every round.  One JSON line; --json writes it to a
file as well.
python tools/zoom_bench.py [--frames 256] [--rounds 5] [--launches 200] [--kernel-only] [--json profiles/zoom_bench.json]"""
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
    n, fs = 32, 256
    xx = torch.linspace(-1, 1, fs, device="cuda")
    g = torch.stack(torch.meshgrid(xx, xx, indexing="xy"), -1)
    fields = torch.stack([g * (1.05 + 0.002 * i) + 0.01 for i in range(n)]).contiguous()
    out, dst = torch.empty_like(fields), torch.empty_like(fields)
    unc = torch.empty((n,), device="cuda", dtype=torch.int32)
    k = [0.9 - 0.01 * i for i in range(n)]   # a window per frame
    h0, w0 = FRAME
    wins = [(0.5 * w0 * (1 - v), 0.5 * w0 * (1 + v), 0.5 * h0 * (1 - v), 0.5 * h0 * (1 + v)) for v in k]
    coef = PF.zoom_coefficients(PF._zoom_windows(wins, n, FRAME), FRAME, (fs, fs)).cuda()
    variants = {
        "copy_ms": lambda: dst.copy_(fields),
        "zoom_ms": lambda: PF._field_zoom(fields, coef, FRAME, False, "bilinear", out, None),
        "zoom_count_ms": lambda: PF._field_zoom(fields, coef, FRAME, False, "bilinear", out, unc),
    }
    for fn in variants.values():   # warm-up: code objects, the allocator
        events_ms(fn, 10)
    samples = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            samples[name].append(events_ms(fn, launches))
    res = {"fields": "%d x %d x %d x 2 fp32" % (n, fs, fs), "bytes_moved": 2 * fields.numel() * 4, "rounds": rounds, "launches_per_round": launches}
    for name, v in samples.items():
        res[name] = {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
    res["zoom_over_copy"] = round(res["zoom_ms"]["median"] / res["copy_ms"]["median"], 3)
    res["zoom_count_over_copy"] = round(res["zoom_count_ms"]["median"] / res["copy_ms"]["median"], 3)
    res["zoom_GBps"] = round(res["bytes_moved"] / res["zoom_ms"]["median"] / 1e6, 1)
    return res


def stream_part(T, rounds):
    from pwstablenet_amd.lib.networks_cascading import define_G
    from pwstablenet_amd.stream import VideoStabilizer
    with contextlib.redirect_stdout(sys.stderr):
        net = define_G(31, 2, 64, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=64)})
    net = net.cuda()
    base = synth.smooth_frames_u8(1, T, FRAME[0], FRAME[1], 3)[0]
    u8_h = torch.from_numpy(np.repeat(base[..., None], 3, -1)).pin_memory()
    vs = VideoStabilizer(net, batch=32, swap_rb=True)
    rows = []
    for in_flight in (1, 2):
        modes = {"none": {}, "zoom_auto": {"zoom": "auto"}, "crop_auto": {"crop": "auto"}}
        times = {name: [] for name in modes}
        row = {"in_flight": in_flight}

        def run(kw):
            vs.run_video(u8_h, chunk=32, half_size_output=True, in_flight=in_flight, **kw)
            torch.cuda.synchronize()
        try:
            for kw in modes.values():   # warm-up of every path
                run(kw)
            for _ in range(rounds):
                for name, kw in modes.items():
                    t0 = time.perf_counter()
                    run(kw)
                    times[name].append(time.perf_counter() - t0)
                    if name == "zoom_auto":
                        window = [round(v, 3) for v in vs.zoom_windows[0]]
        except ValueError as e:   # (a clip whose fields give no crop window)
            row["error"] = str(e)[:200]
            rows.append(row)
            continue
        for name, v in times.items():
            row[name + "_fps"] = {"median": round(T / statistics.median(v), 1), "min": round(T / max(v), 1), "max": round(T / min(v), 1)}
        row["zoom_auto_over_crop_auto"] = round(row["zoom_auto_fps"]["median"] / row["crop_auto_fps"]["median"], 3)
        row["zoom_auto_over_none"] = round(row["zoom_auto_fps"]["median"] / row["none_fps"]["median"], 3)
        row["zoom_window"] = window
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
        sys.exit("zoom_bench: no GPU visible (timings are taken on the device only)")
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
