#!/usr/bin/env python3
"""What crop-bounded smoothing costs and does, in one session on one MI355X (tools/wobble_bench.py's shape and helpers): (a)
pws_field_reach on (128, 256, 256, 2) fields over the rectangle of the centred 0.9 window at 16 and at 32 levels, beside what gives the same
counts today -- levels + 1 launches of pws_field_compose with its uncovered count -- and beside a device copy of the field bytes: us per
launch from device events, the candidates alternating over several rounds, median and range, us per frame; pws_path_levels and
pws_path_limit beside them; (b) host-to-host frames/s of run_video on a pinned-host 1280x720 textured shaky clip (BGR and NV12, in_flight
1 and 2) with smooth=4, without and with max_crop=0.05, alternating, every repeat next to the best, and limited / unlimited as a ratio;
(c) with --parent DIR (a checkout of the parent commit with its library built): the default path and smooth=4 of DIR's package and of
this one -- which leaves max_crop at None -- in child processes of this session, ordered parent, head, parent, head: both are held to the
spread of the parent's own repeats; (d) effect: a 1280x720 textured clip with little shake and one frame displaced by 60 pixels, under an
identity generator (smooth=4 is then a classical stabiliser), at zoom=0.95 without and with max_crop=0.05: the worst zoom_uncovered, the
frames with wedges, the strengths and the stability score.  The engine clock and the host's load average go into the result.  One JSON
line, also written to --json.
python tools/path_limit_bench.py [--frames 128] [--parent DIR] [--json profiles/path_limit_bench.json]"""
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
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bicubic_warp_bench import engine_clock, launch_us, timed  # noqa: E402
from path_smooth_bench import _net, textured_clip  # noqa: E402

from pwstablenet_amd import hipabi as A  # noqa: E402
from pwstablenet_amd import synth  # noqa: E402

SIGMA = 4.0
CROP = 0.05
FRAME = (720, 1280)


def kernel_rows(n=128, size=256, rounds=3):
    from pwstablenet_amd import stream as S
    xx = torch.linspace(-1, 1, size, device="cuda")
    g = torch.stack(torch.meshgrid(xx, xx, indexing="xy"), -1)
    field = torch.stack([g * (0.98 + 0.0002 * i) + 0.004 * torch.sin(3.0 * g.flip(-1) + 0.1 * i) for i in range(n)]).contiguous()
    out = torch.empty_like(field)
    unc = torch.empty((n,), device="cuda", dtype=torch.int32)
    rs = np.random.RandomState(0)
    th, sc = np.deg2rad(rs.normal(0, 0.4, n)), np.exp(rs.normal(0, 0.01, n))
    d = torch.from_numpy(np.stack([sc * np.cos(th), -sc * np.sin(th), rs.normal(0, 30, n), sc * np.sin(th), sc * np.cos(th), rs.normal(0, 18, n)], 1)).cuda()
    rect = S.limit_rectangle(0.9, FRAME, (size, size))
    L, res = A.lib(), {}
    fns = {"device_copy": lambda: out.copy_(field)}
    keep = []
    for levels in (16, 32):
        table = torch.empty((n, levels + 1, 6), device="cuda", dtype=torch.float64)
        counts = torch.empty((n, levels + 1), device="cuda", dtype=torch.int32)
        need = torch.empty((n,), device="cuda", dtype=torch.int32)
        strength = torch.empty((n,), device="cuda", dtype=torch.float64)
        d_out = torch.empty((n, 6), device="cuda", dtype=torch.float64)
        A.check(L.pws_path_levels(A.ptr(d), n, levels, A.ptr(table), A.current_stream()))
        rows_l = [table[:, l].contiguous() for l in range(levels + 1)]
        keep.append((table, counts, need, strength, d_out, rows_l))

        def reach(table=table, counts=counts, levels=levels):
            A.check(L.pws_field_reach(A.ptr(field), n, size, size, A.ptr(table), levels, None, 0.0, rect[0], rect[1], rect[2], rect[3], FRAME[0], FRAME[1],
                                      0, 0, A.ptr(counts), A.current_stream()))

        def composes(rows_l=rows_l):   # the only way to these counts without the kernel (and over the whole lattice, not the rectangle)
            for row in rows_l:
                A.check(L.pws_field_compose(A.ptr(field), n, size, size, A.ptr(row), A.ptr(out), FRAME[0], FRAME[1], 0, 0, A.ptr(unc), A.current_stream()))
        fns["field_reach_%d_levels" % levels] = reach
        fns["field_compose_counted_x%d" % (levels + 1)] = composes
        fns["path_levels_%d" % levels] = lambda table=table, levels=levels: A.check(L.pws_path_levels(A.ptr(d), n, levels, A.ptr(table), A.current_stream()))
        fns["path_limit_%d" % levels] = lambda counts=counts, levels=levels, need=need, strength=strength, d_out=d_out: A.check(
            L.pws_path_limit(A.ptr(d), A.ptr(counts), n, levels, 1.0 / 12, A.ptr(need), A.ptr(strength), A.ptr(d_out), A.current_stream()))
        reach()
        res["frames_limited_at_%d_levels" % levels] = int((counts[:, levels] > 0).sum())
    us = {k: [] for k in fns}
    for _ in range(rounds):   # alternating
        for k, fn in fns.items():
            us[k].append(launch_us(fn, iters=20 if "compose" in k else 100))
    nodes = (rect[1] - rect[0] + 1) * (rect[3] - rect[2] + 1)
    res.update({"fields": [n, size, size, 2], "frame": "1280x720", "window": 0.9, "rectangle": list(rect), "rectangle_nodes": nodes, "rounds": rounds,
                "field_bytes": field.numel() * 4})
    for k, v in us.items():
        med = statistics.median(v)
        res[k + "_us"] = round(med, 2)
        res[k + "_us_range"] = [round(min(v), 2), round(max(v), 2)]
        res[k + "_us_per_frame"] = round(med / n, 3)
    for levels in (16, 32):
        r = res["field_reach_%d_levels_us" % levels]
        res["reach_%d_over_composes" % levels] = round(r / res["field_compose_counted_x%d_us" % (levels + 1)], 3)
        res["reach_%d_over_copy" % levels] = round(r / res["device_copy_us"], 3)
        res["reach_%d_ns_per_node_and_level" % levels] = round(r * 1e3 / (n * nodes * (levels + 1)), 4)
        res["reach_%d_field_gb_per_second_if_read_once" % levels] = round(field.numel() * 4 / (r * 1e-6) / 1e9, 1)
    return res


def _identity_net():
    """tests/test_hip_smooth_stream.py's identity generator (ngf 16, align_corners=True): smooth=4 is then a classical stabiliser."""
    from pwstablenet_amd.lib.networks_cascading import define_G
    sd = {"module." + k: torch.from_numpy(v.copy()) for k, v in synth.make_weights("W1", seed=123, ngf=16)}
    sd["module.linear.mpconv.0.weight"].zero_()
    sd["module.linear.mpconv.0.bias"].copy_(torch.from_numpy(synth.IDENTITY_THETA))
    sd["module.out.mpconv.0.weight"].zero_()
    sd["module.out.mpconv.0.bias"].zero_()
    with contextlib.redirect_stdout(sys.stderr):
        g = define_G(31, 2, 16, "normal", 0.02)
    g.load_state_dict(sd)
    g.module.align_corners = True
    return g.cuda()


def effect(T=96, jolt=(48, 60.0), zoom=0.95):
    from pwstablenet_amd.stream import VideoStabilizer
    clip = textured_clip(T, FRAME[0], FRAME[1], seed=5, sigma=1.0, jolt=jolt)[0].cuda()
    net = _identity_net()
    out = {"frames": T, "frame": "1280x720", "jitter_px": 1.0, "jolt": {"frame": jolt[0], "pixels": jolt[1]}, "zoom": zoom, "smooth": SIGMA, "max_crop": CROP}
    for name, crop in (("unlimited", None), ("limited", CROP)):
        vs = VideoStabilizer(net, batch=8, smooth=SIGMA, metrics=True, max_crop=crop)
        vs.run_video(clip, chunk=32, zoom=zoom)
        rep = vs.stability_report()
        row = {"zoom_uncovered_max": int(vs.zoom_uncovered.max()), "frames_with_wedges": int((vs.zoom_uncovered > 0).sum()),
               "stability_in": round(rep["stability_in"]["stability"], 4), "stability_out": round(rep["stability_out"]["stability"], 4),
               "correction_px_max": round(float(vs.smooth_correction[:, [2, 5]].abs().max()), 2)}
        if crop is not None:
            s = vs.limit_strength
            row.update({"strength_min": round(float(s.min()), 4), "strength_mean": round(float(s.mean()), 4), "frames_below_1": int((s < 1).sum()),
                        "limit_uncovered_max": int(vs.limit_uncovered.max()), "need_min": int(vs.limit_need.min())})
        out[name] = row
    return out


def stream_rows(T, repeats=3):
    from pwstablenet_amd.stream import VideoStabilizer
    clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in textured_clip(T, 720, 1280))))
    net = _net()
    vss = {None: VideoStabilizer(net, batch=32, smooth=SIGMA), CROP: VideoStabilizer(net, batch=32, smooth=SIGMA, max_crop=CROP)}
    rows = []
    for in_flight in (1, 2):
        row = {"in_flight": in_flight}
        fps = {(fmt, c): [] for fmt in clips for c in vss}
        for _ in range(repeats):   # alternating
            for (fmt, c), v in fps.items():
                v.append(T / timed(lambda: vss[c].run_video(clips[fmt], chunk=32, half_size_output=True, in_flight=in_flight, pixel_format=fmt)))
        for (fmt, c), v in fps.items():
            name = "%s_%s" % (fmt, "limited" if c else "unlimited")
            row[name + "_fps"] = round(max(v), 1)
            row[name + "_fps_median"] = round(statistics.median(v), 1)
            row[name + "_fps_all"] = [round(x, 1) for x in v]
        for fmt in clips:
            row[fmt + "_limited_over_unlimited"] = round(row[fmt + "_limited_fps"] / row[fmt + "_unlimited_fps"], 3)
        rows.append(row)
    vs = vss[CROP]
    return rows, {"strength_min": round(float(vs.limit_strength.min()), 4), "frames_below_1": int((vs.limit_strength < 1).sum()),
                  "limit_uncovered_max": int(vs.limit_uncovered.max())}


def parent_rows(T, repeats=3):
    """the worker of part (c): run_video as the parent knows it -- the default path and smooth=4, no max_crop argument"""
    from pwstablenet_amd.stream import VideoStabilizer
    clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in textured_clip(T, 720, 1280))))
    net = _net()
    out = {}
    for name, vs in (("default", VideoStabilizer(net, batch=32)), ("smooth4", VideoStabilizer(net, batch=32, smooth=SIGMA))):
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
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "path_limit_bench.json"))
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(parent_rows(a.frames)))
        return
    def done(part):   # (each part takes a minute or more: say where the session is)
        print("path_limit_bench: %s done" % part, file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(0), "load_avg_before": [round(v, 1) for v in os.getloadavg()]}
    res["kernels"] = kernel_rows(n=a.frames)
    res["sclk_mhz_after_kernel_loops"] = engine_clock()
    done("(a) kernels")
    res["effect"] = effect()
    done("(d) effect")
    rows, clip_facts = stream_rows(a.frames)
    done("(b) run_video")
    res["stream"] = {"frames": a.frames, "source": "1280x720 pinned host, textured, jitter 3 px", "output": "640x360", "math": "fp32", "ngf": 64, "batch": 32,
                     "chunk": 32, "smooth": SIGMA, "max_crop": CROP, "rows": rows, "last_limited_run": clip_facts}
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
