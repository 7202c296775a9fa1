#!/usr/bin/env python3
"""What the stability report costs, in one session on one MI355X: (a) pws_block_motion and pws_motion_fit alone on (33, 256, 256) planes: us
per launch from device events (tools/bicubic_warp_bench.py's method; the two alternate over several rounds, median and range reported), us
per frame pair, and the dword SAD instructions per second that the block search's time amounts to -- counted from shapes: pairs x 196
blocks x 1089 candidates x 64 dwords; (b) host-to-host frames/s of run_video on a pinned-host 1280x720 clip as BGR and as NV12 at in_flight
1 and 2 with metrics off and on, alternating (fp32 generator, ngf 64), every repeat next to the best, and on / off as a ratio; (c) with
--parent DIR (a checkout of the parent commit with its library built): the default path, metrics off, of DIR's package and of this one in
child processes of this session, ordered parent, head, parent, head -- the default path is held to the spread of its own repeats.  The
engine clock (rocm-smi, read right after the timed loops) and the host's load average go into the result.  One JSON line, also written to
--json.
python tools/stability_metrics_bench.py [--frames 128] [--parent DIR] [--json profiles/stability_metrics_bench.json]"""
import argparse
import contextlib
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
import torch  # noqa: E402
from bicubic_warp_bench import clip, engine_clock, launch_us, timed  # noqa: E402

from pwstablenet_amd import hipabi as A  # noqa: E402
from pwstablenet_amd import synth  # noqa: E402


def kernel_rows(n=33, size=256, radius=16, rounds=3):
    # noise planes, each the one before it rolled by a few pixels: every block has a true match, so the fit does its whole work
    g = torch.Generator().manual_seed(0)
    planes = [torch.rand((size, size), generator=g) * 2 - 1]
    for _ in range(n - 1):
        planes.append(torch.roll(planes[-1], [int(v) for v in torch.randint(-12, 13, (2,), generator=g)], (0, 1)))
    planes = torch.stack(planes).cuda().contiguous()
    nb = (size - 2 * radius) // 16
    mv = torch.empty((n, nb, nb, 2), device="cuda", dtype=torch.int16)
    sad = torch.empty((n, nb, nb, 5), device="cuda", dtype=torch.int32)
    act = torch.empty((n, nb, nb), device="cuda", dtype=torch.int32)
    motion = torch.empty((n, 4), device="cuda", dtype=torch.float64)
    inl = torch.empty((n,), device="cuda", dtype=torch.int32)
    L = A.lib()
    fns = {"block_motion": lambda: A.check(L.pws_block_motion(A.ptr(planes), n, size, size, radius, A.ptr(mv), A.ptr(sad), A.ptr(act), A.current_stream())),
           "motion_fit": lambda: A.check(L.pws_motion_fit(A.ptr(mv), A.ptr(sad), A.ptr(act), n, size, size, radius, 0, A.ptr(motion), A.ptr(inl),
                                                          A.current_stream()))}   # (every block of the rolled noise planes is fitted)
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            us[k].append(launch_us(fn, iters=200))
    pairs = n - 1
    sads = pairs * nb * nb * (2 * radius + 1) ** 2 * 64
    rows = {"planes": [n, size, size], "radius": radius, "blocks": nb * nb, "pairs": pairs, "launches_per_round": 200, "rounds": rounds,
            "dword_sads_per_launch": sads}
    for k, v in us.items():
        med = statistics.median(v)
        rows[k + "_us"] = round(med, 2)
        rows[k + "_us_range"] = [round(min(v), 2), round(max(v), 2)]
        rows[k + "_us_per_pair"] = round(med / pairs, 3)
        rows[k + "_us_per_pair_range"] = [round(min(v) / pairs, 3), round(max(v) / pairs, 3)]
    rows["dword_sads_per_second"] = round(sads / (rows["block_motion_us"] * 1e-6), 0)
    return rows


def _net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    with contextlib.redirect_stdout(sys.stderr):
        net = define_G(31, 2, 64, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=64)})
    return net.cuda()


def stream_rows(T, repeats=3):
    from pwstablenet_amd.stream import VideoStabilizer
    clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in clip(T, 720, 1280))))
    vs = VideoStabilizer(_net(), batch=32)
    rows = []
    for in_flight in (1, 2):
        row = {"in_flight": in_flight}
        fps = {(fmt, m): [] for fmt in clips for m in (False, True)}
        for _ in range(repeats):   # alternating
            for (fmt, m), v in fps.items():
                v.append(T / timed(lambda: vs.run_video(clips[fmt], chunk=32, half_size_output=True, in_flight=in_flight, pixel_format=fmt, metrics=m)))
        for (fmt, m), v in fps.items():
            row["%s_%s_fps" % (fmt, "on" if m else "off")] = round(max(v), 1)
            row["%s_%s_fps_median" % (fmt, "on" if m else "off")] = round(statistics.median(v), 1)
            row["%s_%s_fps_all" % (fmt, "on" if m else "off")] = [round(x, 1) for x in v]
        for fmt in clips:
            row[fmt + "_on_over_off"] = round(row[fmt + "_on_fps"] / row[fmt + "_off_fps"], 3)
        rows.append(row)
    return rows


def default_path_rows(T, repeats=3):
    """the worker of part (c): run_video as the parent knows it -- no metrics argument"""
    from pwstablenet_amd.stream import VideoStabilizer
    clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in clip(T, 720, 1280))))
    vs = VideoStabilizer(_net(), batch=32)
    out = {}
    for in_flight in (1, 2):
        for fmt, c in clips.items():
            v = [T / timed(lambda: vs.run_video(c, chunk=32, half_size_output=True, in_flight=in_flight, pixel_format=fmt)) for _ in range(repeats)]
            out["%s_in_flight_%d_fps_all" % (fmt, in_flight)] = [round(x, 1) for x in v]
            out["%s_in_flight_%d_fps" % (fmt, in_flight)] = round(max(v), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, library built: part (c)")
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "stability_metrics_bench.json"))
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(default_path_rows(a.frames)))
        return
    res = {"device": torch.cuda.get_device_name(0), "load_avg_before": [round(v, 1) for v in os.getloadavg()]}
    res["kernels"] = kernel_rows()
    res["sclk_mhz_after_kernel_loops"] = engine_clock()
    res["stream"] = {"frames": a.frames, "source": "1280x720 pinned host", "output": "640x360", "math": "fp32", "ngf": 64, "batch": 32, "chunk": 32,
                     "rows": stream_rows(a.frames)}
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
        keys = [k for k in runs[0] if k.endswith("_fps")]
        summary = {}
        for k in keys:
            p = [x for r in runs if r["build"] == "parent" for x in r[k + "_all"]]
            h = [x for r in runs if r["build"] == "head" for x in r[k + "_all"]]
            summary[k] = {"parent_best": max(p), "head_best": max(h), "parent_range": [min(p), max(p)], "head_range": [min(h), max(h)],
                          "head_over_parent_best": round(max(h) / max(p), 3), "head_over_parent_median": round(statistics.median(h) / statistics.median(p), 3)}
        res["default_path"] = {"order": [r["build"] for r in runs], "runs": runs, "summary": summary}
        res["sclk_mhz_after_default_path"] = engine_clock()
    res["load_avg_after"] = [round(v, 1) for v in os.getloadavg()]
    line = json.dumps(res)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
