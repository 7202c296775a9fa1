#!/usr/bin/env python3
"""What the fused warp costs per packed YUV format, in one process on one box: functional.upsample_grid_sample_yuv on 8 frames of 1280x720 of
all ten packed formats -- 4:2:0 (nv12, i420, p010, i010), 4:2:2 (nv16, i422, p210, i210) and 4:4:4 (i444, i410) -- bilinear and bicubic, on
the same 8 stabiliser-like fields: us per launch from device events (tools/yuv16_stream_bench.py's method: the kernels alternate over several
rounds, median and range reported), the algorithmic frame traffic in bytes per pixel (in + out: 2 x samples per pixel x bytes per sample),
the fraction of 8 TB/s it reaches, and the ratio to the 4:2:0 format of the same depth and plane order.  No speed is promised for the new
formats: the file records what they cost.  The engine clock (rocm-smi, read right after the timed loops) and the host's load average go
into the result.  One JSON line, also written to --json.
python tools/chroma_formats_bench.py [--rounds 5] [--json profiles/chroma_formats_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from yuv16_stream_bench import engine_clock, launch_us  # noqa: E402

from pwstablenet_amd import functional as PF  # noqa: E402

BASE = {"nv16": "nv12", "i422": "i420", "i444": "i420", "p210": "p010", "i210": "i010", "i410": "i010"}


def rows(n=8, h=720, w=1280, rounds=5, iters=1000):
    xx = torch.linspace(-1, 1, 256, device="cuda")
    g = torch.stack(torch.meshgrid(xx, xx, indexing="xy"), -1)
    field = torch.stack([g * (1.02 + 0.002 * i) + 0.01 for i in range(n)]).contiguous()
    fns, bpp = {}, {}
    for name in PF.PACKED_FORMATS:
        fmt = PF.lookup_format(name)
        shape = (n, fmt.packed_rows(h), w)
        if fmt.dtype == torch.uint8:
            src = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda")
        else:   # 10-bit samples in the format's placement (layout 0: the high bits)
            src = (torch.randint(0, 1024, shape, dtype=torch.int32, device="cuda") << (6 if fmt.layout == 0 else 0)).to(torch.uint16)
        out = torch.empty_like(src)
        bpp[name] = 2.0 * fmt.packed_rows(h) / h * src.element_size()
        for mode in PF.INTERPOLATIONS:
            fns[name, mode] = lambda name=name, src=src, out=out, mode=mode: PF.upsample_grid_sample_yuv(src, field, name, out=out, mode=mode)
    us = {k: [] for k in fns}
    for _ in range(rounds):   # the kernels alternate, so that a drift of clock or load hits all of them
        for k, fn in fns.items():
            us[k].append(launch_us(fn, iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    res = {"launches_per_round": iters, "rounds": rounds, "formats": {}}
    for name in PF.PACKED_FORMATS:
        fmt = PF.lookup_format(name)
        row = {"chroma": ("4:2:0", "4:2:2", "4:4:4")[fmt.chroma], "dtype": str(fmt.dtype)[6:], "layout": fmt.layout, "bytes_per_pixel": bpp[name]}
        for mode in PF.INTERPOLATIONS:
            row[mode + "_us"] = round(med[name, mode], 2)
            row[mode + "_us_range"] = [round(min(us[name, mode]), 2), round(max(us[name, mode]), 2)]
            row[mode + "_frac_8TBs"] = round(bpp[name] * n * h * w / (med[name, mode] * 1e-6) / 8e12, 3)
            if name in BASE:
                row["%s_over_%s" % (mode, BASE[name])] = round(med[name, mode] / med[BASE[name], mode], 3)
        res["formats"][name] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "chroma_formats_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "load_avg_before": [round(v, 1) for v in os.getloadavg()]}
    res["warp"] = dict(frames=8, size="1280x720", **rows(rounds=a.rounds))
    res["sclk_mhz_after_warp_loops"] = engine_clock()
    res["load_avg_after"] = [round(v, 1) for v in os.getloadavg()]
    line = json.dumps(res)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
