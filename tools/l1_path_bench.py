#!/usr/bin/env python3
"""What the L1-optimal path costs, in one session on one MI355X: (a) pws_l1_path on one scene of 128 and of 2 048 frames (a shaky pan in
frame pixels, 1280 x 720, reach 0.1, the paper's weights) beside pws_path_smooth at sigma 4 on the same motion: us per call from device events
(tools/bicubic_warp_bench.py's method; the two alternate over several rounds, median and range reported), the Newton steps each component
took, and from them the us per Newton step of the slowest component -- the single-lane band solve's cost as measured, not estimated;
(b) host-to-host frames/s of run_video on a pinned-host 1280x720 textured shaky clip (BGR, in_flight 1 and 2) with smooth="l1" and smooth=4,
alternating (fp32 generator, ngf 64), every repeat next to the best; (c) with --parent DIR (a checkout of the parent commit with its library
built): the default path and smooth=4 of DIR's package and of this one in child processes of this session, ordered parent, head, parent,
head, the parent's own repeat spread beside the ratio.  The engine clock (rocm-smi, read right after the timed loops) and the host's load
average go into the result.  One JSON line, also written to --json.
python tools/l1_path_bench.py [--frames 128] [--parent DIR] [--json profiles/l1_path_bench.json]"""
import argparse
import ctypes
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


def kernel_rows(sizes=(128, 2048), rounds=3):
    from pwstablenet_amd.motion import _l1_bounds
    L = A.lib()
    bound = (ctypes.c_double * 4)(*_l1_bounds(0.1, (720, 1280), "l1_path_bench"))
    weights = (ctypes.c_double * 3)(10.0, 1.0, 100.0)
    rows = {"frame": "1280x720", "reach": 0.1, "weights": [10.0, 1.0, 100.0], "rounds": rounds}
    for n in sizes:
        rs = np.random.RandomState(0)
        motion = torch.from_numpy(np.stack([np.ones(n), 0.003 * rs.normal(size=n), 12 + 8 * rs.normal(size=n), -5 + 8 * rs.normal(size=n)], 1)).cuda()
        path = torch.empty((n, 4), device="cuda", dtype=torch.float64)
        corr = torch.empty((n, 6), device="cuda", dtype=torch.float64)
        info = torch.empty((4, 4), device="cuda", dtype=torch.float64)
        nbytes = int(L.pws_l1_path_workspace(n))
        ws = torch.empty((nbytes // 8,), device="cuda", dtype=torch.float64)
        fns = {"l1_path": lambda: A.check(L.pws_l1_path(A.ptr(motion), n, bound, weights, A.ptr(path), A.ptr(corr), A.ptr(info), A.ptr(ws), nbytes,
                                                       A.current_stream())),
               "path_smooth_sigma4": lambda: A.check(L.pws_path_smooth(A.ptr(motion), n, 4.0, A.ptr(path), A.ptr(corr), A.current_stream()))}
        us = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                us[k].append(launch_us(fn, iters=200 if k != "l1_path" else 20))
        fns["l1_path"]()
        steps = info.cpu().numpy()
        row = {"workspace_bytes": nbytes, "newton_steps": [int(v) for v in steps[:, 0]], "converged": [int(v) for v in steps[:, 3]]}
        for k, v in us.items():
            row[k + "_us"] = round(statistics.median(v), 2)
            row[k + "_us_range"] = [round(min(v), 2), round(max(v), 2)]
        row["l1_us_per_newton_step_of_the_slowest_component"] = round(row["l1_path_us"] / max(1, max(row["newton_steps"])), 2)
        row["l1_over_path_smooth"] = round(row["l1_path_us"] / row["path_smooth_sigma4_us"], 1)
        rows["frames_%d" % n] = row
    return rows


def stream_rows(T, repeats=3):
    from pwstablenet_amd.stream import VideoStabilizer
    clip = textured_clip(T, 720, 1280)[0].pin_memory()
    net = _net()
    vss = {"l1": VideoStabilizer(net, batch=32, smooth="l1"), "smooth4": VideoStabilizer(net, batch=32, smooth=4.0)}
    rows = []
    for in_flight in (1, 2):
        row = {"in_flight": in_flight}
        fps = {k: [] for k in vss}
        for _ in range(repeats):   # alternating
            for k, v in fps.items():
                v.append(T / timed(lambda: vss[k].run_video(clip, chunk=32, half_size_output=True, in_flight=in_flight)))
        for k, v in fps.items():
            row["bgr24_%s_fps" % k] = round(max(v), 1)
            row["bgr24_%s_fps_all" % k] = [round(x, 1) for x in v]
        row["l1_over_smooth4"] = round(row["bgr24_l1_fps"] / row["bgr24_smooth4_fps"], 3)
        rows.append(row)
    vs = vss["l1"]
    d, info = vs.smooth_correction.cpu().numpy(), vs.smooth_l1_info.cpu().numpy()
    return rows, {"fitted_pairs": int((vs.smooth_inliers > 0).sum()), "largest_shift_px": round(float(np.abs(d[:, [2, 5]]).max()), 2),
                  "uncovered_nodes_mean": round(float(vs.smooth_uncovered.float().mean()), 1), "newton_steps": [int(v) for v in info[0, :, 0]],
                  "converged": [int(v) for v in info[0, :, 3]]}


def worker_rows(T, repeats=3):
    """the worker of part (c): run_video as the parent knows it -- the default path and smooth=4"""
    from pwstablenet_amd.stream import VideoStabilizer
    clip = textured_clip(T, 720, 1280)[0].pin_memory()
    net = _net()
    out = {}
    for name, vs in (("default", VideoStabilizer(net, batch=32)), ("smooth4", VideoStabilizer(net, batch=32, smooth=4.0))):
        for in_flight in (1, 2):
            v = [T / timed(lambda: vs.run_video(clip, chunk=32, half_size_output=True, in_flight=in_flight)) for _ in range(repeats)]
            out["%s_in_flight_%d_fps_all" % (name, in_flight)] = [round(x, 1) for x in v]
            out["%s_in_flight_%d_fps" % (name, in_flight)] = round(max(v), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, library built: part (c)")
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "l1_path_bench.json"))
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(worker_rows(a.frames)))
        return
    res = {"device": torch.cuda.get_device_name(0), "load_avg_before": [round(v, 1) for v in os.getloadavg()]}
    res["kernels"] = kernel_rows()
    res["sclk_mhz_after_kernel_loops"] = engine_clock()
    rows, clip_facts = stream_rows(a.frames)
    res["stream"] = {"frames": a.frames, "source": "1280x720 pinned host, textured, jitter 3 px", "output": "640x360", "math": "fp32", "ngf": 64, "batch": 32,
                     "chunk": 32, "rows": rows, "last_l1_run": clip_facts}
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
                          "parent_repeat_spread": round((max(p) - min(p)) / max(p), 4), "head_over_parent_best": round(max(h) / max(p), 3),
                          "head_over_parent_median": round(statistics.median(h) / statistics.median(p), 3)}
        res["default_path_and_smooth4"] = {"order": [r["build"] for r in runs], "runs": runs, "summary": summary}
        res["sclk_mhz_after_parent_runs"] = engine_clock()
    res["load_avg_after"] = [round(v, 1) for v in os.getloadavg()]
    line = json.dumps(res)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
