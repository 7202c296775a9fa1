#!/usr/bin/env python3
"""What borders="keep" costs, in one process on the same box: (a) functional.keep_borders_ on 8 warped frames of 1280x720 of every integer
format (BGR bytes, NV12 / I420, P010 / I010) next to that format's bilinear warp on the same 8 stabiliser-like fields (a 2 % zoom-out: a rim
of uncovered pixels on every side): us per launch from device events (tools/bicubic_warp_bench.py's method; the kernels alternate over several
rounds, median and range reported) and the ratio keep / warp; (b) host-to-host frames/s of run_video on a pinned-host 1280x720 clip as BGR and
as NV12 with borders "black" and "keep", at in_flight 1 and 2 (fp32 generator, ngf 64).  The engine clock (rocm-smi, read right after the timed
loops) and the host's load average go into the result.  One JSON line, also written to --json.
python tools/keep_borders_bench.py [--frames 128] [--pass-only] [--json profiles/keep_borders_bench.json]"""
import argparse
import contextlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from bicubic_warp_bench import clip, engine_clock, launch_us, timed  # noqa: E402

from pwstablenet_amd import functional as PF  # noqa: E402
from pwstablenet_amd import synth  # noqa: E402

BORDERS = ("black", "keep")


def pass_rows(n=8, h=720, w=1280, rounds=3):
    xx = torch.linspace(-1, 1, 256, device="cuda")
    g = torch.stack(torch.meshgrid(xx, xx, indexing="xy"), -1)
    field = torch.stack([g * (1.02 + 0.002 * i) + 0.01 for i in range(n)]).contiguous()
    bgr = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
    yuv = torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8, device="cuda")
    y16 = torch.randint(0, 1024, (n, h * 3 // 2, w), dtype=torch.int32, device="cuda")
    src = {"bgr_u8": bgr, "nv12": yuv, "i420": yuv, "p010": (y16 << 6).to(torch.uint16), "i010": y16.to(torch.uint16)}
    out = {k: torch.empty_like(v) for k, v in src.items()}
    fns = {}
    for fmt in src:
        pf = "bgr24" if fmt == "bgr_u8" else fmt
        if fmt == "bgr_u8":
            fns[fmt, "warp"] = lambda: PF.upsample_grid_sample_u8(bgr, field, out=out["bgr_u8"])
        elif fmt in ("nv12", "i420"):
            fns[fmt, "warp"] = lambda fmt=fmt: PF.upsample_grid_sample_yuv420(yuv, field, fmt, out=out[fmt])
        else:
            fns[fmt, "warp"] = lambda fmt=fmt: PF.upsample_grid_sample_yuv420_16(src[fmt], field, fmt, out=out[fmt])
        fns[fmt, "warp"]()   # (the pass then runs on warped frames; it rewrites the same bytes every launch)
        fns[fmt, "keep"] = lambda fmt=fmt, pf=pf: PF.keep_borders_(out[fmt], field, src[fmt][0], pf, initial_is_source=True)
    us = {k: [] for k in fns}
    for _ in range(rounds):   # the kernels alternate, so that a drift of clock or load hits all of them
        for k, fn in fns.items():
            us[k].append(launch_us(fn))
    rows = {"launches_per_round": 500, "rounds": rounds}
    med = {k: statistics.median(v) for k, v in us.items()}
    for (fmt, m), v in med.items():
        rows["%s_%s_us" % (fmt, m)] = round(v, 2)
        rows["%s_%s_us_range" % (fmt, m)] = [round(min(us[fmt, m]), 2), round(max(us[fmt, m]), 2)]
    for fmt in src:
        rows[fmt + "_keep_over_warp"] = round(med[fmt, "keep"] / med[fmt, "warp"], 3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--pass-only", action="store_true")
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "keep_borders_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "load_avg_before": [round(v, 1) for v in os.getloadavg()]}
    res["pass"] = dict(frames=8, size="1280x720", **pass_rows())
    res["sclk_mhz_after_pass_loops"] = engine_clock()
    if not a.pass_only:
        from pwstablenet_amd.lib.networks_cascading import define_G
        from pwstablenet_amd.stream import VideoStabilizer
        with contextlib.redirect_stdout(sys.stderr):
            net = define_G(31, 2, 64, "normal", 0.02)
        net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=64)})
        net = net.cuda()
        T = a.frames
        clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in clip(T, 720, 1280))))
        vs = {b: VideoStabilizer(net, batch=32, borders=b) for b in BORDERS}
        rows = []
        for in_flight in (1, 2):
            row = {"in_flight": in_flight}
            fps = {(fmt, b): [] for fmt in clips for b in BORDERS}
            for _ in range(2):   # alternating
                for (fmt, b), v in fps.items():
                    v.append(T / timed(lambda: vs[b].run_video(clips[fmt], chunk=32, half_size_output=True, in_flight=in_flight, pixel_format=fmt)))
            for (fmt, b), v in fps.items():
                row["%s_%s_fps" % (fmt, b)] = round(max(v), 1)
                row["%s_%s_fps_all" % (fmt, b)] = [round(x, 1) for x in v]
            for fmt in clips:
                row[fmt + "_keep_over_black"] = round(row[fmt + "_keep_fps"] / row[fmt + "_black_fps"], 3)
            rows.append(row)
        res["stream"] = {"frames": T, "source": "1280x720 pinned host", "output": "640x360", "math": "fp32", "ngf": 64, "batch": 32, "chunk": 32,
                         "rows": rows}
        res["sclk_mhz_after_stream"] = engine_clock()
    res["load_avg_after"] = [round(v, 1) for v in os.getloadavg()]
    line = json.dumps(res)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
