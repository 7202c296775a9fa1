#!/usr/bin/env python3
"""What the rolling-shutter estimate costs, in one session on one MI355X (tools/path_limit_bench.py's shape and helpers): (a)
pws_shutter_terms on the blocks, motion and rates that the device measured on a shaky textured clip of 256 x 256 planes (radius 16: 196
blocks a pair), in plane pixels and at a 1280x720 frame's pixel scale, beside pws_motion_fit_scaled on the same blocks and
pws_shutter_estimate on the terms: us per launch from device events, the candidates alternating over several rounds, median and range, us
per pair; (b) host-to-host frames/s of run_video on a pinned-host 1280x720 textured shaky clip (BGR and NV12, in_flight 1 and 2) with
smooth=4 and rolling_shutter="auto" against the same call with the number that "auto" chose, alternating, every repeat next to the best:
the difference is the estimate plus the one host read; (c) with --parent DIR (a checkout of the parent commit with its library built): the
default path and smooth=4 of DIR's package and of this one in child processes of this session, ordered parent, head, parent, head: both are
held to the spread of the parent's own repeats.  The engine clock and the host's load average go into the result.  One JSON line, also
written to --json.
python tools/shutter_estimate_bench.py [--frames 128] [--parent DIR] [--json profiles/shutter_estimate_bench.json]"""
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
import torch  # noqa: E402
from bicubic_warp_bench import engine_clock, launch_us, timed  # noqa: E402
from path_limit_bench import parent_rows  # noqa: E402
from path_smooth_bench import _net, textured_clip  # noqa: E402

from pwstablenet_amd import hipabi as A  # noqa: E402

SIGMA = 4.0
FRAME = (720, 1280)


def kernel_rows(n=32, size=256, rounds=3):
    from pwstablenet_amd import stream as S
    planes = S.window_planes(textured_clip(n, FRAME[0], FRAME[1], seed=5, sigma=3.0)[0].cuda(), size)
    L, res, fns, keep = A.lib(), {}, {}, []
    for name, scale in (("plane_pixels", None), ("frame_pixels", (FRAME[1] / size, FRAME[0] / size))):
        motion, inl, mv, sad, act = S.global_motion(planes, return_blocks=True, pixel_scale=scale)
        rates = S.shutter_rates(motion)
        est, terms = S.estimate_rolling_shutter(motion, mv, sad, act, (size, size), pixel_scale=scale, return_terms=True)
        sx, sy = scale or (1.0, 1.0)
        keep.append((motion, inl, mv, sad, act, rates, est, terms))
        res[name + "_estimate"] = [round(v, 5) for v in est.tolist()]
        res[name + "_pairs_with_blocks"] = int((terms[:, 3] > 0).sum())
        fns["shutter_terms_" + name] = lambda mv=mv, sad=sad, act=act, motion=motion, rates=rates, terms=terms, sx=sx, sy=sy: A.check(
            L.pws_shutter_terms(A.ptr(mv), A.ptr(sad), A.ptr(act), A.ptr(motion), A.ptr(rates), n, size, size, 16, 2000, sx, sy, size * sy, A.ptr(terms),
                                A.current_stream()))
        if scale is not None:
            scratch, sinl = torch.empty_like(motion), torch.empty_like(inl)
            keep.append((scratch, sinl))
            fns["motion_fit_scaled"] = lambda mv=mv, sad=sad, act=act, sx=sx, sy=sy: A.check(
                L.pws_motion_fit_scaled(A.ptr(mv), A.ptr(sad), A.ptr(act), n, size, size, 16, 2000, sx, sy, A.ptr(scratch), A.ptr(sinl), A.current_stream()))
            fns["shutter_estimate"] = lambda terms=terms, est=est: A.check(L.pws_shutter_estimate(A.ptr(terms), n, A.ptr(est), A.current_stream()))
            fns["shutter_rates"] = lambda motion=motion, rates=rates: A.check(L.pws_shutter_rates(A.ptr(motion), n, A.ptr(rates), A.current_stream()))
    us = {k: [] for k in fns}
    for _ in range(rounds):   # alternating
        for k, fn in fns.items():
            us[k].append(launch_us(fn, iters=200))
    res.update({"planes": [n, size, size], "radius": 16, "blocks_per_pair": 196, "rounds": rounds, "launches_per_round": 200})
    for k, v in us.items():
        med = statistics.median(v)
        res[k + "_us"] = round(med, 2)
        res[k + "_us_range"] = [round(min(v), 2), round(max(v), 2)]
        res[k + "_us_per_pair"] = round(med / n, 3)
    return res


def stream_rows(T, repeats=3):
    from pwstablenet_amd.stream import VideoStabilizer
    clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in textured_clip(T, FRAME[0], FRAME[1]))))
    net = _net()
    rows, chosen = [], {}
    for fmt, c in clips.items():   # the number that "auto" chooses on this clip: what the fixed-r call is given
        vs = VideoStabilizer(net, batch=32, smooth=SIGMA, rolling_shutter="auto")
        vs.run_video(c, chunk=32, half_size_output=True, pixel_format=fmt)
        chosen[fmt] = {"used": vs.rolling_shutter_used, "estimate": vs.shutter_estimate.tolist()}
    for in_flight in (1, 2):
        row = {"in_flight": in_flight}
        vss = {(fmt, mode): VideoStabilizer(net, batch=32, smooth=SIGMA, rolling_shutter="auto" if mode == "auto" else chosen[fmt]["used"])
               for fmt in clips for mode in ("number", "auto")}
        fps = {k: [] for k in vss}
        for _ in range(repeats):   # alternating
            for (fmt, mode), v in fps.items():
                v.append(T / timed(lambda: vss[(fmt, mode)].run_video(clips[fmt], chunk=32, half_size_output=True, in_flight=in_flight, pixel_format=fmt)))
        for (fmt, mode), v in fps.items():
            name = "%s_%s" % (fmt, mode)
            row[name + "_fps"] = round(max(v), 1)
            row[name + "_fps_median"] = round(statistics.median(v), 1)
            row[name + "_fps_all"] = [round(x, 1) for x in v]
        for fmt in clips:
            row[fmt + "_auto_over_number"] = round(row[fmt + "_auto_fps"] / row[fmt + "_number_fps"], 3)
            row[fmt + "_auto_minus_number_ms_per_clip"] = round(1e3 * T * (1.0 / row[fmt + "_auto_fps"] - 1.0 / row[fmt + "_number_fps"]), 3)
        rows.append(row)
    return rows, chosen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, library built: part (c)")
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "shutter_estimate_bench.json"))
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(parent_rows(a.frames)))
        return

    def done(part):   # (each part takes a minute or more: say where the session is)
        print("shutter_estimate_bench: %s done" % part, file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(0), "load_avg_before": [round(v, 1) for v in os.getloadavg()]}
    res["kernels"] = kernel_rows()
    res["sclk_mhz_after_kernel_loops"] = engine_clock()
    done("(a) kernels")
    rows, chosen = stream_rows(a.frames)
    done("(b) run_video")
    res["stream"] = {"frames": a.frames, "source": "1280x720 pinned host, textured, jitter 3 px", "output": "640x360", "math": "fp32", "ngf": 64, "batch": 32,
                     "chunk": 32, "smooth": SIGMA, "chosen": chosen, "rows": rows}
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
            done("(c) worker %d of 4 (%s)" % (len(runs), who))
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
