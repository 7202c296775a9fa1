#!/usr/bin/env python3
"""What wobble suppression costs and does, in one session on one MI355X (tools/rolling_shutter_bench.py's shape and helpers): (a)
pws_field_wobble on (128, 256, 256, 2) fields at sigma 2 and 5 (R = 6 and 15), with and without the statistics, beside pws_field_rigid and a
device copy of the same bytes: us per launch from device events, the kernels alternating over several rounds, median and range, us per
frame; (b) host-to-host frames/s of run_video on a pinned-host 1280x720 textured shaky clip (BGR and NV12, in_flight 1 and 2) without and
with wobble=2, alternating, every repeat next to the best, and filtered / plain as a ratio -- wobble takes the two-pass route, so it also
pays the second upload of the frames; (c) with --parent DIR (a checkout of the parent commit with its library built): the default path and
smooth=4 of DIR's package and of this one -- which leaves wobble at 0 -- in child processes of this session, ordered parent, head, parent,
head: both are held to the spread of the parent's own repeats; (d) effectiveness on synthetic fields: a homography path plus a static
distortion plus white per-frame wobble of a known amplitude, the wobble's RMS before and after sigma 2 at interior frames beside the
float64 prediction sqrt(sum g^2) / sum g.  The engine clock and the host's load average go into the result.  One JSON line, also written
to --json.
python tools/wobble_bench.py [--frames 128] [--parent DIR] [--json profiles/wobble_bench.json]"""
import argparse
import json
import math
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

SIGMA = 2.0
FRAME = (720, 1280)


def _path(n):
    """(n, 9) float64: a smooth homography path (rotation, scale, translation, a little perspective)."""
    m = np.empty((n, 9))
    for t in range(n):
        a, s = np.deg2rad(1.5 * np.sin(0.11 * t)), 1 + 0.02 * np.cos(0.07 * t)
        m[t] = [s * np.cos(a), -s * np.sin(a), 0.03 * np.sin(0.05 * t), s * np.sin(a), s * np.cos(a), 0.02 * np.cos(0.09 * t), 0.005, -0.004, 1.0]
    return m


def synthetic_fields(n, size, amplitude, seed=0):
    """(field, m, clean): clean = the path's own positions P (pws_field_rigid at rigidity 1) plus a static smooth distortion; field = clean
    plus white noise of RMS ``amplitude`` per frame and node."""
    from pwstablenet_amd import functional as PF
    m = torch.from_numpy(_path(n)).cuda()
    P = PF.rigid_fields(torch.zeros((n, size, size, 2), device="cuda"), m, FRAME, 1.0)
    xx = torch.linspace(-1, 1, size, device="cuda")
    u, v = xx[None, :], xx[:, None]
    static = 0.01 * torch.stack([torch.sin(2.5 * v) * torch.cos(1.5 * u), torch.cos(2.0 * u) * torch.sin(3.0 * v)], -1)
    clean = P + static
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return clean + amplitude * torch.randn(clean.shape, generator=gen, device="cuda"), m, clean


def kernel_rows(n=128, size=256, rounds=3):
    field, m, _ = synthetic_fields(n, size, 1e-3)
    field = field.contiguous()
    out = torch.empty_like(field)
    st_f = torch.empty((n,), device="cuda", dtype=torch.float32)
    st_i = torch.empty((n,), device="cuda", dtype=torch.int32)
    L = A.lib()

    def wobble(sigma, stats):
        f, i = (st_f, st_i) if stats else (None, None)
        return lambda: A.check(L.pws_field_wobble(A.ptr(field), n, size, size, A.ptr(m), sigma, FRAME[0], FRAME[1], A.ptr(out), A.ptr(f), A.ptr(i),
                                                  A.current_stream()))

    def rigid(stats):
        f, i = (st_f, st_i) if stats else (None, None)
        return lambda: A.check(L.pws_field_rigid(A.ptr(field), n, size, size, A.ptr(m), 1.0, FRAME[0], FRAME[1], A.ptr(out), A.ptr(f), A.ptr(i),
                                                 A.current_stream()))
    fns = {"field_wobble_sigma2": wobble(2.0, False), "field_wobble_sigma5": wobble(5.0, False), "field_wobble_sigma2_stats": wobble(2.0, True),
           "field_wobble_sigma5_stats": wobble(5.0, True), "field_rigid": rigid(False), "field_rigid_stats": rigid(True),
           "device_copy": lambda: out.copy_(field)}
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            us[k].append(launch_us(fn, iters=100))
    moved = 2 * field.numel() * 4   # the fields once in and once out
    res = {"fields": [n, size, size, 2], "frame": "1280x720", "launches_per_round": 100, "rounds": rounds, "field_bytes_in_and_out": moved}
    for k, v in us.items():
        med = statistics.median(v)
        res[k + "_us"] = round(med, 2)
        res[k + "_us_range"] = [round(min(v), 2), round(max(v), 2)]
        res[k + "_us_per_frame"] = round(med / n, 3)
    for k in ("field_wobble_sigma2", "field_wobble_sigma5"):
        res[k + "_over_rigid"] = round(res[k + "_us"] / res["field_rigid_us"], 3)
        res[k + "_over_copy"] = round(res[k + "_us"] / res["device_copy_us"], 3)
    return res


def effectiveness(n=96, size=256, amplitude=1e-3):
    from pwstablenet_amd import functional as PF
    field, m, clean = synthetic_fields(n, size, amplitude, seed=1)
    out, removed, unfit = PF.wobble_fields(field, m, FRAME, SIGMA, return_stats=True)
    R = int(math.ceil(3 * SIGMA))
    before = float((field - clean)[R:n - R].double().pow(2).mean().sqrt())
    after = float((out - clean)[R:n - R].double().pow(2).mean().sqrt())
    k = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2 * SIGMA * SIGMA)).astype(np.float32).astype(np.float64)
    return {"fields": [n, size, size, 2], "sigma": SIGMA, "injected_rms": amplitude, "wobble_rms_before": before, "wobble_rms_after": after,
            "ratio": round(after / before, 4), "predicted_ratio": round(float(np.sqrt((g * g).sum()) / g.sum()), 4),
            "removed_px_median": round(float(removed.median()), 3), "unfit_nodes": int(unfit.sum())}


def stream_rows(T, repeats=3):
    from pwstablenet_amd.stream import VideoStabilizer
    clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in textured_clip(T, 720, 1280))))
    net = _net()
    vss = {0.0: VideoStabilizer(net, batch=32), SIGMA: VideoStabilizer(net, batch=32, wobble=SIGMA)}
    rows = []
    for in_flight in (1, 2):
        row = {"in_flight": in_flight}
        fps = {(fmt, s): [] for fmt in clips for s in vss}
        for _ in range(repeats):   # alternating
            for (fmt, s), v in fps.items():
                v.append(T / timed(lambda: vss[s].run_video(clips[fmt], chunk=32, half_size_output=True, in_flight=in_flight, pixel_format=fmt)))
        for (fmt, s), v in fps.items():
            name = "%s_%s" % (fmt, "wobble" if s else "plain")
            row[name + "_fps"] = round(max(v), 1)
            row[name + "_fps_median"] = round(statistics.median(v), 1)
            row[name + "_fps_all"] = [round(x, 1) for x in v]
        for fmt in clips:
            row[fmt + "_wobble_over_plain"] = round(row[fmt + "_wobble_fps"] / row[fmt + "_plain_fps"], 3)
        rows.append(row)
    vs = vss[SIGMA]
    return rows, {"removed_px_median": round(float(vs.wobble_removed.median()), 3), "removed_px_max": round(float(vs.wobble_removed.max()), 3),
                  "unfit_nodes": int(vs.wobble_unfit.sum())}


def parent_rows(T, repeats=3):
    """the worker of part (c): run_video as the parent knows it -- the default path and smooth=4, no wobble argument"""
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
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "wobble_bench.json"))
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(parent_rows(a.frames)))
        return
    res = {"device": torch.cuda.get_device_name(0), "load_avg_before": [round(v, 1) for v in os.getloadavg()]}
    res["kernels"] = kernel_rows(n=a.frames)
    res["sclk_mhz_after_kernel_loops"] = engine_clock()
    res["effectiveness"] = effectiveness()
    rows, clip_facts = stream_rows(a.frames)
    res["stream"] = {"frames": a.frames, "source": "1280x720 pinned host, textured, jitter 3 px", "output": "640x360", "math": "fp32", "ngf": 64, "batch": 32,
                     "chunk": 32, "wobble": SIGMA, "rows": rows, "last_filtered_run": clip_facts}
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
