#!/usr/bin/env python3
"""What deblurring costs, in one session on one MI355X: (a) functional.deblur_frames on 16 frames of 1280 x 720 at R = 2, bgr24 and nv12, once
with gains that give every frame four donors and once with none (a copy): us per launch from device events (tools/bicubic_warp_bench.py's
method; the cases alternate over several rounds, median and range reported), us per frame, and the share of the HBM peak (8 TB/s) that the
bytes counted from shapes give -- every blended sample read once, written once and read once more per donor; chroma once in, once out;
frame_sharpness beside them; (b) host-to-host frames/s of run_video on a pinned-host 1280 x 720 textured shaky clip (BGR and NV12) with
deblur=0 and deblur=2, alternating (fp32 generator, ngf 64), every repeat next to the best -- deblur=2 takes the two-pass route, so it also
pays the second upload of the frames; (c) with --parent DIR (a checkout of the parent commit with its library built): the default path and
smooth=4 of DIR's package and of this one in child processes of this session, ordered parent, head, parent, head -- both are held to the
spread of the parent's own repeats.  The engine clock (rocm-smi, read right after the timed loops) and the host's load average go into
the result.  One JSON line, also written to --json.
python tools/deblur_bench.py [--frames 96] [--parent DIR] [--json profiles/deblur_bench.json]"""
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

HBM_PEAK = 8.0e12   # bytes per second, the specification's


def kernel_rows(n=16, h=720, w=1280, R=2, rounds=3):
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import stream as S
    bgr, nv12 = (c.cuda() for c in textured_clip(n, h, w))
    K = 2 * R + 1
    rs = np.random.RandomState(0)
    maps = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (n, K, 1))
    th = np.deg2rad(0.1)
    for k in range(-R, R + 1):   # a near-translation: 1.3 pixel a frame, a tenth of a degree
        maps[:, R + k] = [np.cos(k * th), -np.sin(k * th), 1.3 * k + 0.21, np.sin(k * th), np.cos(k * th), -0.7 * k + 0.37]
    maps[:, R] = [1.0, 0, 0, 0, 1.0, 0]
    m = n - 2 * R   # the frames that have all their neighbours are written
    maps = torch.from_numpy(maps[R:n - R]).cuda()
    lend = rs.uniform(0.2, 0.8, (m, K)).astype(np.float32)
    lend[:, R] = 0.0
    gains = {"donors": torch.from_numpy(lend).cuda(), "copy": torch.zeros((m, K), device="cuda")}
    clips = {"bgr24": bgr, "nv12": nv12}
    outs = {f: torch.empty_like(c) for f, c in clips.items()}
    fns = {}
    for fmt, c in clips.items():
        for name, g in gains.items():
            fns["%s_%s" % (fmt, name)] = (lambda c=c, g=g, fmt=fmt: PF.deblur_frames(c, maps, g, R, n - R, fmt, 4.0, out=outs[fmt][:n - 2 * R]))
        fns["%s_sharpness" % fmt] = (lambda c=c, fmt=fmt: S.frame_sharpness(c, fmt))
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            us[k].append(launch_us(fn, iters=100))
    rows = {"frames_per_launch": {"deblur": n - 2 * R, "sharpness": n}, "frame": "%dx%d" % (w, h), "radius": R, "launches_per_round": 100, "rounds": rounds,
            "hbm_peak_bytes_per_second": HBM_PEAK}
    for k, v in us.items():
        fmt, what = k.split("_")
        blended = h * w * (3 if fmt == "bgr24" else 1)      # bytes of a frame that are blended; nv12 copies h w / 2 more
        copied = 0 if fmt == "bgr24" else h * w // 2
        per = n if what == "sharpness" else n - 2 * R
        moved = {"donors": blended * (2 + 2 * R) + 2 * copied, "copy": 2 * (blended + copied), "sharpness": blended}[what]
        med = statistics.median(v)
        rows[k] = {"us_per_launch": round(med, 2), "us_range": [round(min(v), 2), round(max(v), 2)], "us_per_frame": round(med / per, 2),
                   "bytes_per_frame_from_shapes": moved, "share_of_hbm_peak": round(moved * per / (med * 1e-6) / HBM_PEAK, 4)}
    return rows


def stream_rows(T, repeats=3):
    from pwstablenet_amd.stream import VideoStabilizer
    clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in textured_clip(T, 720, 1280))))
    net = _net()
    vss = {0: VideoStabilizer(net, batch=32), 2: VideoStabilizer(net, batch=32, deblur=2)}
    row = {}
    fps = {(fmt, r): [] for fmt in clips for r in vss}
    for _ in range(repeats):   # alternating
        for (fmt, r), v in fps.items():
            v.append(T / timed(lambda: vss[r].run_video(clips[fmt], chunk=32, half_size_output=True, pixel_format=fmt)))
    for (fmt, r), v in fps.items():
        name = "%s_deblur%d" % (fmt, r)
        row[name + "_fps"] = round(max(v), 1)
        row[name + "_fps_median"] = round(statistics.median(v), 1)
        row[name + "_fps_all"] = [round(x, 1) for x in v]
    for fmt in clips:
        row[fmt + "_deblur_over_plain"] = round(row[fmt + "_deblur2_fps"] / row[fmt + "_deblur0_fps"], 3)
    vs = vss[2]
    facts = {"frames_with_donors": int((vs.deblur_donors > 0).sum()), "donors_mean": round(float(vs.deblur_donors.float().mean()), 2)}
    return row, facts


def parent_rows(T, repeats=3):
    """the worker of part (c): run_video as the parent knows it -- the default path and smooth=4"""
    from pwstablenet_amd.stream import VideoStabilizer
    clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in textured_clip(T, 720, 1280))))
    net = _net()
    out = {}
    for name, vs in (("default", VideoStabilizer(net, batch=32)), ("smooth4", VideoStabilizer(net, batch=32, smooth=4.0))):
        for fmt, c in clips.items():
            v = [T / timed(lambda: vs.run_video(c, chunk=32, half_size_output=True, pixel_format=fmt)) for _ in range(repeats)]
            out["%s_%s_fps_all" % (fmt, name)] = [round(x, 1) for x in v]
            out["%s_%s_fps" % (fmt, name)] = round(max(v), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, library built: part (c)")
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "deblur_bench.json"))
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(parent_rows(a.frames)))
        return
    res = {"device": torch.cuda.get_device_name(0), "load_avg_before": [round(v, 1) for v in os.getloadavg()]}
    res["kernels"] = kernel_rows()
    res["sclk_mhz_after_kernel_loops"] = engine_clock()
    row, facts = stream_rows(a.frames)
    res["stream"] = {"frames": a.frames, "source": "1280x720 pinned host, textured, jitter 3 px", "output": "640x360", "math": "fp32", "ngf": 64, "batch": 32,
                     "chunk": 32, "radius": 2, "sensitivity": 4.0, "in_flight": 1, "row": row, "last_deblurred_run": facts}
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
                          "parent_spread": round(max(p) / min(p) - 1.0, 3), "head_over_parent_best": round(max(h) / max(p), 3),
                          "head_over_parent_median": round(statistics.median(h) / statistics.median(p), 3)}
        res["against_parent"] = {"order": [r["build"] for r in runs], "runs": runs, "summary": summary}
        res["sclk_mhz_after_parent"] = engine_clock()
    res["load_avg_after"] = [round(v, 1) for v in os.getloadavg()]
    line = json.dumps(res)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
