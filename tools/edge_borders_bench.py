#!/usr/bin/env python3
"""What edge="clamp" / "mirror" costs, in one process on the same box: (a) functional.edge_borders_ on 8 warped frames of 1280x720 of every
integer format -- BGR bytes and the ten packed YUV formats -- for both edges and both interpolations, next to that format's warp of the same
interpolation and next to functional.keep_borders_, on tools/mosaic_borders_bench.py's 8 stabiliser-like fields (a 1 % zoom-out under a shift
that changes from frame to frame: a rim of uncovered pixels on every side): us per launch from device events (tools/bicubic_warp_bench.py's
method; the kernels alternate over several rounds, median and range reported), the ratios edge / warp and edge / keep, and the share of Y
positions the bilinear margin leaves uncovered; (b) host-to-host frames/s of run_video on a pinned-host 1280x720 clip as BGR and as NV12 with
edge "pad" and "mirror" at in_flight 1 and 2 (fp32 generator, ngf 64, borders "black").  The engine clock (rocm-smi, read right after the
timed loops) and the host's load average go into the result.  One JSON line, also written to --json.
python tools/edge_borders_bench.py [--frames 128] [--pass-only] [--json profiles/edge_borders_bench.json]"""
import argparse
import contextlib
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from bicubic_warp_bench import clip, engine_clock, launch_us, timed  # noqa: E402

from pwstablenet_amd import functional as PF  # noqa: E402
from pwstablenet_amd import synth  # noqa: E402

EDGES = ("clamp", "mirror")
FORMATS = ("bgr24",) + PF.PACKED_FORMATS


def pass_rows(n=8, h=720, w=1280, rounds=3):
    xx = torch.linspace(-1, 1, 256, device="cuda")
    g = torch.stack(torch.meshgrid(xx, xx, indexing="xy"), -1)
    shift = [torch.tensor([0.015 * math.cos(2.1 * i), 0.015 * math.sin(1.7 * i)], device="cuda") for i in range(n)]
    field = torch.stack([g * 1.01 + shift[i] for i in range(n)]).contiguous()
    ix, iy = (field[..., 0] + 1) * w / 2 - 0.5, (field[..., 1] + 1) * h / 2 - 0.5   # (the field's nodes, align_corners=False: the rim's width)
    uncovered = float(((ix < 0) | (ix > w - 1) | (iy < 0) | (iy > h - 1)).float().mean())
    src, out, fns = {}, {}, {}
    for name in FORMATS:
        fmt = PF.lookup_format(name)
        shape = (n, h, w, 3) if fmt.hwc else (n, fmt.packed_rows(h), w)
        if fmt.dtype == torch.uint8:
            src[name] = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda")
        else:
            v = torch.randint(0, 1024, shape, dtype=torch.int32, device="cuda")
            src[name] = (v << 6 if fmt.layout == 0 else v).to(torch.uint16)
        out[name] = torch.empty_like(src[name])
        for mode in PF.INTERPOLATIONS:
            fns[name, mode, "warp"] = lambda name=name, fmt=fmt, mode=mode: PF.warp(src[name], field, fmt, out=out[name], mode=mode)
            fns[name, mode, "keep"] = lambda name=name, mode=mode: PF.keep_borders_(out[name], field, src[name][0], name, initial_is_source=True, mode=mode)
            for edge in EDGES:   # (the passes run on warped frames and rewrite the same bytes every launch)
                fns[name, mode, edge] = lambda name=name, mode=mode, edge=edge: PF.edge_borders_(out[name], src[name], field, edge, name, mode=mode)
        fns[name, "bilinear", "warp"]()
    us = {k: [] for k in fns}
    for _ in range(rounds):   # the kernels alternate, so that a drift of clock or load hits all of them
        for k, fn in fns.items():
            us[k].append(launch_us(fn))
    rows = {"launches_per_round": 500, "rounds": rounds, "uncovered_share_of_field_nodes": round(uncovered, 5)}
    med = {k: statistics.median(v) for k, v in us.items()}
    for (name, mode, what), v in med.items():
        rows["%s_%s_%s_us" % (name, mode, what)] = round(v, 2)
        rows["%s_%s_%s_us_range" % (name, mode, what)] = [round(min(us[name, mode, what]), 2), round(max(us[name, mode, what]), 2)]
    for name in FORMATS:
        for mode in PF.INTERPOLATIONS:
            for edge in EDGES:
                rows["%s_%s_%s_over_warp" % (name, mode, edge)] = round(med[name, mode, edge] / med[name, mode, "warp"], 3)
                rows["%s_%s_%s_over_keep" % (name, mode, edge)] = round(med[name, mode, edge] / med[name, mode, "keep"], 3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--pass-only", action="store_true")
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "edge_borders_bench.json"))
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
        vs = {e: VideoStabilizer(net, batch=32, edge=e) for e in ("pad", "mirror")}
        rows = []
        for in_flight in (1, 2):
            row = {"in_flight": in_flight}
            fps = {(fmt, e): [] for fmt in clips for e in vs}
            for _ in range(2):   # alternating
                for (fmt, e), v in fps.items():
                    v.append(T / timed(lambda: vs[e].run_video(clips[fmt], chunk=32, half_size_output=True, in_flight=in_flight, pixel_format=fmt)))
            for (fmt, e), v in fps.items():
                row["%s_%s_fps" % (fmt, e)] = round(max(v), 1)
                row["%s_%s_fps_all" % (fmt, e)] = [round(x, 1) for x in v]
            for fmt in clips:
                row[fmt + "_mirror_over_pad"] = round(row[fmt + "_mirror_fps"] / row[fmt + "_pad_fps"], 3)
            rows.append(row)
        res["stream"] = {"frames": T, "source": "1280x720 pinned host", "output": "640x360", "math": "fp32", "ngf": 64, "batch": 32, "chunk": 32,
                         "borders": "black", "rows": rows}
        res["sclk_mhz_after_stream"] = engine_clock()
    res["load_avg_after"] = [round(v, 1) for v in os.getloadavg()]
    line = json.dumps(res)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
