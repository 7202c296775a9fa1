#!/usr/bin/env python3
"""What rolling-shutter correction costs, in one session on one MI355X (tools/path_smooth_bench.py's shape and helpers): (a)
pws_field_compose_rows (r = 0.8, rates that are not zero) beside pws_field_compose on the same (32, 256, 256, 2) fields and corrections of
a 1280x720 frame, with and without the uncovered count: us per launch from device events, the kernels alternating over several rounds,
median and range, us per frame; pws_shutter_rates on a scene of --frames frames beside them; (b) host-to-host frames/s of run_video on
a pinned-host 1280x720 textured shaky clip (BGR and NV12, in_flight 1 and 2) with smooth=4 alone and with rolling_shutter=0.8, alternating,
every repeat next to the best, and corrected / smooth as a ratio; (c) with --parent DIR (a checkout of the parent commit with its library
built): the default path (no smooth) and smooth=4 of DIR's package and of this one -- which leaves rolling_shutter at 0 -- in child
processes of this session, ordered parent, head, parent, head: both are held to the spread of the parent's own repeats.  The engine
clock and the host's load average go into the result.  One JSON line, also written to --json.
python tools/rolling_shutter_bench.py [--frames 128] [--parent DIR] [--json profiles/rolling_shutter_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _package_root(argv):
    return argv[argv.index("--package-root") + 1] if "--package-root" in argv else ROOT


sys.path.insert(0, HERE)
sys.path.insert(0, _package_root(sys.argv))   # (a worker of part (c) imports the package of the checkout it measures)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bicubic_warp_bench import engine_clock, launch_us, timed  # noqa: E402
from path_smooth_bench import _net, textured_clip  # noqa: E402

from pwstablenet_amd import hipabi as A  # noqa: E402

R = 0.8


def kernel_rows(n=32, size=256, frames=128, rounds=3):
    xx = torch.linspace(-1, 1, size, device="cuda")
    g = torch.stack(torch.meshgrid(xx, xx, indexing="xy"), -1)
    field = torch.stack([g * (1.02 + 0.002 * i) + 0.01 for i in range(n)]).contiguous()
    out = torch.empty_like(field)
    unc = torch.empty((n,), device="cuda", dtype=torch.int32)
    th = np.deg2rad(0.4)
    d = torch.tensor([[1.01 * np.cos(th), -1.01 * np.sin(th), 7.3, 1.01 * np.sin(th), 1.01 * np.cos(th), -4.1]] * n, dtype=torch.float64, device="cuda")
    rs = np.random.RandomState(0)
    motion = torch.from_numpy(np.stack([np.ones(frames), 0.003 * rs.normal(size=frames), 12 + 8 * rs.normal(size=frames),
                                        -5 + 8 * rs.normal(size=frames)], 1)).cuda()
    rates_all = torch.empty((frames, 2, 4), device="cuda", dtype=torch.float64)
    L = A.lib()

    def shutter():
        A.check(L.pws_shutter_rates(A.ptr(motion), frames, A.ptr(rates_all), A.current_stream()))
    shutter()
    rates = rates_all[:n].contiguous()

    def compose(u):
        return lambda: A.check(L.pws_field_compose(A.ptr(field), n, size, size, A.ptr(d), A.ptr(out), 720, 1280, 0, 0, A.ptr(u), A.current_stream()))

    def rows(u):
        return lambda: A.check(L.pws_field_compose_rows(A.ptr(field), n, size, size, A.ptr(d), A.ptr(rates), R, A.ptr(out), 720, 1280, 0, 0, A.ptr(u),
                                                        A.current_stream()))
    fns = {"field_compose": compose(None), "field_compose_rows": rows(None), "field_compose_counted": compose(unc), "field_compose_rows_counted": rows(unc),
           "shutter_rates": shutter}
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            us[k].append(launch_us(fn, iters=200))
    res = {"fields": [n, size, size, 2], "frame": "1280x720", "rolling_shutter": R, "launches_per_round": 200, "rounds": rounds, "shutter_rates_frames": frames}
    for k, v in us.items():
        med = statistics.median(v)
        res[k + "_us"] = round(med, 2)
        res[k + "_us_range"] = [round(min(v), 2), round(max(v), 2)]
        res[k + "_us_per_frame"] = round(med / (frames if k == "shutter_rates" else n), 3)
    res["rows_over_compose"] = round(res["field_compose_rows_us"] / res["field_compose_us"], 3)
    res["rows_over_compose_counted"] = round(res["field_compose_rows_counted_us"] / res["field_compose_counted_us"], 3)
    return res


def stream_rows(T, repeats=3):
    from pwstablenet_amd.stream import VideoStabilizer
    clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in textured_clip(T, 720, 1280))))
    net = _net()
    vss = {0.0: VideoStabilizer(net, batch=32, smooth=4.0), R: VideoStabilizer(net, batch=32, smooth=4.0, rolling_shutter=R)}
    rows = []
    for in_flight in (1, 2):
        row = {"in_flight": in_flight}
        fps = {(fmt, r): [] for fmt in clips for r in vss}
        for _ in range(repeats):   # alternating
            for (fmt, r), v in fps.items():
                v.append(T / timed(lambda: vss[r].run_video(clips[fmt], chunk=32, half_size_output=True, in_flight=in_flight, pixel_format=fmt)))
        for (fmt, r), v in fps.items():
            name = "%s_%s" % (fmt, "corrected" if r else "smooth")
            row[name + "_fps"] = round(max(v), 1)
            row[name + "_fps_median"] = round(statistics.median(v), 1)
            row[name + "_fps_all"] = [round(x, 1) for x in v]
        for fmt in clips:
            row[fmt + "_corrected_over_smooth"] = round(row[fmt + "_corrected_fps"] / row[fmt + "_smooth_fps"], 3)
        rows.append(row)
    rt = vss[R].shutter_rates.cpu().numpy()
    return rows, {"largest_rate_px_per_frame": round(float(np.abs(rt[:, :, 2:]).max()), 2),
                  "uncovered_nodes_mean": round(float(vss[R].smooth_uncovered.float().mean()), 1)}


def parent_rows(T, repeats=3):
    """the worker of part (c): run_video as the parent knows it -- the default path and smooth=4, no rolling_shutter argument"""
    from pwstablenet_amd.stream import VideoStabilizer
    clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in textured_clip(T, 720, 1280))))
    net = _net()
    out = {}
    for name, vs in (("default", VideoStabilizer(net, batch=32)), ("smooth4", VideoStabilizer(net, batch=32, smooth=4.0))):
        for in_flight in (1, 2):
            for fmt, c in clips.items():
                v = [T / timed(lambda: vs.run_video(c, chunk=32, half_size_output=True, in_flight=in_flight, pixel_format=fmt)) for _ in range(repeats)]
                out["%s_%s_in_flight_%d_fps_all" % (name, fmt, in_flight)] = [round(x, 1) for x in v]
                out["%s_%s_in_flight_%d_fps" % (name, fmt, in_flight)] = round(max(v), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, library built: part (c)")
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "rolling_shutter_bench.json"))
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(parent_rows(a.frames)))
        return
    res = {"device": torch.cuda.get_device_name(0), "load_avg_before": [round(v, 1) for v in os.getloadavg()]}
    res["kernels"] = kernel_rows(frames=a.frames)
    res["sclk_mhz_after_kernel_loops"] = engine_clock()
    rows, clip_facts = stream_rows(a.frames)
    res["stream"] = {"frames": a.frames, "source": "1280x720 pinned host, textured, jitter 3 px", "output": "640x360", "math": "fp32", "ngf": 64, "batch": 32,
                     "chunk": 32, "sigma": 4.0, "rolling_shutter": R, "rows": rows, "last_corrected_run": clip_facts}
    res["sclk_mhz_after_stream"] = engine_clock()
    if a.parent:
        torch.cuda.synchronize()
        runs = []
        for who, root in (("parent", a.parent), ("head", ROOT)) * 2:   # fresh child processes, one at a time
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--frames", str(a.frames), "--package-root", os.path.abspath(root)]
            env = {k: v for k, v in os.environ.items() if k != "PWS_LIB_PATH"}   # (every checkout loads its own library)
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=os.path.abspath(root), env=env)
            if out.returncode != 0:
                raise RuntimeError("worker %s failed (rc %d): %s" % (who, out.returncode, out.stderr[-2000:]))
            runs.append(dict(build=who, **json.loads(out.stdout.strip().splitlines()[-1])))
        summary = {}
        for k in [k for k in runs[0] if k.endswith("_fps")]:
            p = [x for r in runs if r["build"] == "parent" for x in r[k + "_all"]]
            h = [x for r in runs if r["build"] == "head" for x in r[k + "_all"]]
            summary[k] = {"parent_best": max(p), "head_best": max(h), "parent_range": [min(p), max(p)], "head_range": [min(h), max(h)],
                          "parent_spread": round(max(p) / min(p) - 1, 4), "head_best_inside_parent_range": bool(min(p) <= max(h)),
                          "head_over_parent_best": round(max(h) / max(p), 3), "head_over_parent_median": round(statistics.median(h) / statistics.median(p), 3)}
        res["against_parent"] = {"order": [r["build"] for r in runs], "runs": runs, "summary": summary}
        res["sclk_mhz_after_against_parent"] = engine_clock()
    res["load_avg_after"] = [round(v, 1) for v in os.getloadavg()]
    line = json.dumps(res)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
