#!/usr/bin/env python3
"""What scene-cut support costs, on one box: (a) pws_scene_change on one chunk of 32 window planes of 256x256 (8.4 MB read): us per launch from
device events (tools/yuv16_stream_bench.py's method: alternating rounds, median and range) and the fraction of 8 TB/s that is, next to the
launch that PRODUCES those planes, pws_gray_area_u8 on 32 frames of 1280x720, in the same rounds; (b) host-to-host frames/s of
run_video(..., half_size_output=True) on a pinned-host 1280x720 uint8 clip (fp32 generator, ngf 64, batch and chunk 32), in_flight 1 and 2,
for scene_cuts=None, scene_cuts="auto" on a one-scene clip and scene_cuts="auto" on a clip with a cut every 64 frames, with the host time
spent in the per-chunk wait for the scores (VideoStabilizer.scene_wait_s).
--parent-tree DIR: a built checkout of the parent commit; its run_video (default arguments) is timed in child processes of this run, two
runs before this tree's and one after, to show the run-to-run spread the default path is held against.  --default-only is what those children
run: it touches nothing the parent lacks.  One JSON line, also written to --json.
python tools/scene_cuts_bench.py [--frames 256] [--parent-tree DIR] [--json profiles/scene_cuts_bench.json]"""
import argparse
import contextlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--tree", default=HERE, help="the checkout whose pwstablenet_amd is imported")
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--json", default=None)
    return ap.parse_args()


ARGS = _args()
sys.path.insert(0, os.path.abspath(ARGS.tree))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402


def timed(fn, reps=2):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def launch_us(fn, iters=500):
    for _ in range(20):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def engine_clock():
    """sclk as `rocm-smi --showclocks` reports it, or None.  A read-only query: this tool never sets or resets anything on the device."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        m = re.search(r"sclk[^\n]*?\((\d+)\s*Mhz\)", out, re.I)
        return int(m.group(1)) if m else None
    except (OSError, subprocess.SubprocessError):
        return None


def clip(T, H, W, scene_len=None, seed=3):
    """A shaky uint8 BGR clip (synth.smooth_frames_u8: one smooth scene under small per-frame translations); scene_len: a new scene every
    scene_len frames."""
    n = scene_len or T
    parts = [synth.smooth_frames_u8(1, min(n, T - s), H, W, seed + 7 * k)[0] for k, s in enumerate(range(0, T, n))]
    base = np.concatenate(parts)
    return torch.from_numpy(np.ascontiguousarray(np.stack([base, base, base], -1)))


def kernel_rows(rounds=5):
    from pwstablenet_amd import hipabi as A
    from pwstablenet_amd.stream import scene_scores, window_planes
    frames = clip(32, 720, 1280).cuda()
    planes = window_planes(frames)
    noise = (torch.rand((32, 256, 256), device="cuda") * 2 - 1).contiguous()        # every lane another bin: the aggregation's worst case
    hist = torch.empty((32, 16, 32), device="cuda", dtype=torch.int32)
    sad = torch.empty((32,), device="cuda", dtype=torch.int32)
    L = A.lib()

    def scene(p):
        return lambda: A.check(L.pws_scene_change(A.ptr(p), 32, 256, 256, A.ptr(hist), A.ptr(sad), A.current_stream()), "pws_scene_change")
    fns = {"scene_change_smooth": scene(planes), "scene_change_noise": scene(noise), "gray_area_u8_720p": lambda: window_planes(frames, out=planes),
           "scene_scores_call": lambda: scene_scores(planes)}
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            us[k].append(launch_us(fn))
    rows = {"planes": "32 x 256 x 256 fp32", "launches_per_round": 500, "rounds": rounds}
    for k in fns:
        rows[k + "_us"] = round(statistics.median(us[k]), 2)
        rows[k + "_us_range"] = [round(min(us[k]), 2), round(max(us[k]), 2)]
    for k in ("scene_change_smooth", "scene_change_noise"):
        rows[k + "_frac_8TBs"] = round(32 * 256 * 256 * 4 / (rows[k + "_us"] * 1e-6) / 8e12, 3)
    rows["scene_over_gray_area"] = round(rows["scene_change_smooth_us"] / rows["gray_area_u8_720p_us"], 3)
    return rows


def make_vs():
    from pwstablenet_amd.lib.networks_cascading import define_G
    from pwstablenet_amd.stream import VideoStabilizer
    with contextlib.redirect_stdout(sys.stderr):
        net = define_G(31, 2, 64, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=64)})
    return VideoStabilizer(net.cuda(), batch=32, swap_rb=True)


def default_rows(vs, one):
    T = one.shape[0]
    return {str(k): [round(T / t, 1) for t in timed(lambda: vs.run_video(one, chunk=32, half_size_output=True, in_flight=k), reps=3)] for k in (1, 2)}


def parent_run(tree, frames):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--default-only", "--tree", tree, "--frames", str(frames)],
                         capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError("parent run failed: " + out.stderr[-2000:])
    return json.loads(out.stdout.strip().splitlines()[-1])["default_fps"]


def main():
    a = ARGS
    T = a.frames
    res = {"device": torch.cuda.get_device_name(0), "load_avg_before": [round(v, 1) for v in os.getloadavg()], "tree": os.path.abspath(a.tree)}
    if a.default_only:
        res["default_fps"] = default_rows(make_vs(), clip(T, 720, 1280).pin_memory())
        print(json.dumps(res))
        return
    res["kernel"] = kernel_rows()
    res["sclk_mhz_after_kernel_loops"] = engine_clock()
    if not a.kernel_only:
        parents = []
        if a.parent_tree:
            parents = [parent_run(a.parent_tree, T), parent_run(a.parent_tree, T)]
        vs = make_vs()
        one, cut = clip(T, 720, 1280).pin_memory(), clip(T, 720, 1280, scene_len=64).pin_memory()
        rows = []
        for in_flight in (1, 2):
            row = {"in_flight": in_flight}
            fps = {"none": [], "auto_one_scene": [], "auto_cut_every_64": []}
            wait = {"auto_one_scene": [], "auto_cut_every_64": []}
            for _ in range(2):   # alternating
                fps["none"] += [T / t for t in timed(lambda: vs.run_video(one, chunk=32, half_size_output=True, in_flight=in_flight), reps=1)]
                for name, src in (("auto_one_scene", one), ("auto_cut_every_64", cut)):
                    fps[name] += [T / t for t in timed(lambda: vs.run_video(src, chunk=32, half_size_output=True, in_flight=in_flight,
                                                                           scene_cuts="auto"), reps=1)]
                    wait[name].append(vs.scene_wait_s)
                    row[name + "_cuts"] = list(vs.scene_cuts)
            for k, v in fps.items():
                row[k + "_fps"], row[k + "_fps_all"] = round(max(v), 1), [round(x, 1) for x in v]
            for k, v in wait.items():
                row[k + "_host_wait_ms"] = [round(x * 1e3, 2) for x in v]
                row[k + "_over_none"] = round(row[k + "_fps"] / row["none_fps"], 4)
            rows.append(row)
        res["stream"] = {"frames": T, "source": "1280x720 uint8 BGR, pinned host", "output": "640x360 (half_size_output)", "math": "fp32", "ngf": 64,
                         "batch": 32, "chunk": 32, "rows": rows}
        res["default_fps_this_tree"] = default_rows(vs, one)
        if a.parent_tree:
            parents.append(parent_run(a.parent_tree, T))
            res["default_fps_parent_runs"] = parents
        res["sclk_mhz_after_stream"] = engine_clock()
    res["load_avg_after"] = [round(v, 1) for v in os.getloadavg()]
    del res["tree"]
    line = json.dumps(res)
    out = a.json or os.path.join(HERE, "profiles", "scene_cuts_bench.json")
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
