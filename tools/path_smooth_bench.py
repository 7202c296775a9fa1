#!/usr/bin/env python3
"""What path smoothing costs, in one session on one MI355X: (a) pws_field_compose beside pws_field_zoom on (32, 256, 256, 2) fields, with and
without the uncovered count: us per launch from device events (tools/bicubic_warp_bench.py's method; the kernels alternate over several
rounds, median and range reported), us per frame, and the bytes per second that moving the field once in and once out amounts to -- counted
from shapes; pws_path_smooth on a scene of --frames frames beside them; (b) host-to-host frames/s of run_video on a pinned-host 1280x720
textured shaky clip (BGR and NV12, in_flight 1 and 2) with smooth=0 and smooth=4, alternating (fp32 generator, ngf 64), every repeat next
to the best, and smooth / plain as a ratio -- smooth=4 takes the two-pass route, so it also pays the second upload of the frames; (c) with
--parent DIR (a checkout of the parent commit with its library built): the default path of DIR's package and of this one in child
processes of this session, ordered parent, head, parent, head -- the default path is held to the spread of its own repeats.  The engine
clock (rocm-smi, read right after the timed loops) and the host's load average go into the result.  One JSON line, also written to --json.
python tools/path_smooth_bench.py [--frames 128] [--parent DIR] [--json profiles/path_smooth_bench.json]"""
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

from pwstablenet_amd import hipabi as A  # noqa: E402
from pwstablenet_amd import synth  # noqa: E402


def textured_clip(T, H, W, seed=3, sigma=3.0, jolt=None):
    """A shaky textured clip, BGR and NV12: twelve sinusoids of 14 to 90 pixels under a pan of (1.0, 0.4) pixel a frame plus Gaussian jitter of
    sigma pixels (the GPU tests' texture: busy enough for global_motion's activity threshold, which synth.smooth_frames_u8 is not).
    jolt = (frame, pixels): that one frame is displaced by so many pixels in x on top (tools/path_limit_bench.py); the draws are unchanged."""
    rs = np.random.RandomState(seed)
    k = 12
    wl, ang, ph = rs.uniform(14.0, 90.0, k), rs.uniform(0, 2 * np.pi, k), rs.uniform(0, 2 * np.pi, k)
    kx, ky = 2 * np.pi / wl * np.cos(ang), 2 * np.pi / wl * np.sin(ang)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    a = (kx[:, None, None].astype(np.float32) * xx + ky[:, None, None].astype(np.float32) * yy + ph[:, None, None].astype(np.float32)).reshape(k, -1)
    sa, ca = np.sin(a), np.cos(a)
    t = np.arange(T)
    tx, ty = 1.0 * t + rs.normal(0, sigma, T), 0.4 * t + rs.normal(0, sigma, T)
    if jolt is not None:
        tx[int(jolt[0])] += float(jolt[1])
    phi = kx[None] * tx[:, None] + ky[None] * ty[:, None]
    v = np.cos(phi).astype(np.float32) @ sa + np.sin(phi).astype(np.float32) @ ca
    base = np.clip(np.rint(127.5 + 127.5 * 0.13 * v), 0, 255).astype(np.uint8).reshape(T, H, W)
    bgr = np.ascontiguousarray(np.repeat(base[..., None], 3, -1))
    nv12 = np.concatenate([(16 + base.astype(np.int32) * 219 // 255).astype(np.uint8), np.full((T, H // 2, W), 128, np.uint8)], 1)
    return torch.from_numpy(bgr), torch.from_numpy(nv12)


def kernel_rows(n=32, size=256, frames=128, rounds=3):
    xx = torch.linspace(-1, 1, size, device="cuda")
    g = torch.stack(torch.meshgrid(xx, xx, indexing="xy"), -1)
    field = torch.stack([g * (1.02 + 0.002 * i) + 0.01 for i in range(n)]).contiguous()
    out = torch.empty_like(field)
    unc = torch.empty((n,), device="cuda", dtype=torch.int32)
    coef = torch.tensor([[3.0, 0.95, 2.0, 0.96]] * n, device="cuda")
    th = np.deg2rad(0.4)
    d = torch.tensor([[1.01 * np.cos(th), -1.01 * np.sin(th), 7.3, 1.01 * np.sin(th), 1.01 * np.cos(th), -4.1]] * n, dtype=torch.float64, device="cuda")
    rs = np.random.RandomState(0)
    motion = torch.from_numpy(np.stack([np.ones(frames), 0.003 * rs.normal(size=frames), 12 + 8 * rs.normal(size=frames),
                                        -5 + 8 * rs.normal(size=frames)], 1)).cuda()
    path = torch.empty((frames, 4), device="cuda", dtype=torch.float64)
    corr = torch.empty((frames, 6), device="cuda", dtype=torch.float64)
    L = A.lib()

    def zoom(u):
        return lambda: A.check(L.pws_field_zoom(A.ptr(field), n, size, size, A.ptr(coef), A.ptr(out), 720, 1280, 0, 0, A.ptr(u), A.current_stream()))

    def compose(u):
        return lambda: A.check(L.pws_field_compose(A.ptr(field), n, size, size, A.ptr(d), A.ptr(out), 720, 1280, 0, 0, A.ptr(u), A.current_stream()))
    fns = {"field_zoom": zoom(None), "field_compose": compose(None), "field_zoom_counted": zoom(unc), "field_compose_counted": compose(unc),
           "path_smooth_sigma4": lambda: A.check(L.pws_path_smooth(A.ptr(motion), frames, 4.0, A.ptr(path), A.ptr(corr), A.current_stream()))}
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            us[k].append(launch_us(fn, iters=200))
    moved = 2 * n * size * size * 2 * 4   # the field once in and once out
    rows = {"fields": [n, size, size, 2], "frame": "1280x720", "launches_per_round": 200, "rounds": rounds, "field_bytes_in_and_out": moved,
            "path_smooth_frames": frames}
    for k, v in us.items():
        med = statistics.median(v)
        per = frames if k.startswith("path") else n
        rows[k + "_us"] = round(med, 2)
        rows[k + "_us_range"] = [round(min(v), 2), round(max(v), 2)]
        rows[k + "_us_per_frame"] = round(med / per, 3)
        if not k.startswith("path"):
            rows[k + "_gb_per_second"] = round(moved / (med * 1e-6) / 1e9, 1)
    rows["compose_over_zoom"] = round(rows["field_compose_us"] / rows["field_zoom_us"], 3)
    return rows


def _net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    with contextlib.redirect_stdout(sys.stderr):
        net = define_G(31, 2, 64, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=64)})
    return net.cuda()


def stream_rows(T, repeats=3):
    from pwstablenet_amd.stream import VideoStabilizer
    clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in textured_clip(T, 720, 1280))))
    net = _net()
    vss = {0.0: VideoStabilizer(net, batch=32), 4.0: VideoStabilizer(net, batch=32, smooth=4.0)}
    rows = []
    for in_flight in (1, 2):
        row = {"in_flight": in_flight}
        fps = {(fmt, s): [] for fmt in clips for s in vss}
        for _ in range(repeats):   # alternating
            for (fmt, s), v in fps.items():
                v.append(T / timed(lambda: vss[s].run_video(clips[fmt], chunk=32, half_size_output=True, in_flight=in_flight, pixel_format=fmt)))
        for (fmt, s), v in fps.items():
            name = "%s_smooth%d" % (fmt, int(s))
            row[name + "_fps"] = round(max(v), 1)
            row[name + "_fps_median"] = round(statistics.median(v), 1)
            row[name + "_fps_all"] = [round(x, 1) for x in v]
        for fmt in clips:
            row[fmt + "_smooth_over_plain"] = round(row[fmt + "_smooth4_fps"] / row[fmt + "_smooth0_fps"], 3)
        rows.append(row)
    vs = vss[4.0]
    d = vs.smooth_correction.cpu().numpy()
    return rows, {"fitted_pairs": int((vs.smooth_inliers > 0).sum()), "largest_shift_px": round(float(np.abs(d[:, [2, 5]]).max()), 2),
                  "uncovered_nodes_mean": round(float(vs.smooth_uncovered.float().mean()), 1)}


def default_path_rows(T, repeats=3):
    """the worker of part (c): run_video as the parent knows it -- no smooth argument"""
    from pwstablenet_amd.stream import VideoStabilizer
    clips = dict(zip(("bgr24", "nv12"), (c.pin_memory() for c in textured_clip(T, 720, 1280))))
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
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "path_smooth_bench.json"))
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(default_path_rows(a.frames)))
        return
    res = {"device": torch.cuda.get_device_name(0), "load_avg_before": [round(v, 1) for v in os.getloadavg()]}
    res["kernels"] = kernel_rows(frames=a.frames)
    res["sclk_mhz_after_kernel_loops"] = engine_clock()
    rows, clip_facts = stream_rows(a.frames)
    res["stream"] = {"frames": a.frames, "source": "1280x720 pinned host, textured, jitter 3 px", "output": "640x360", "math": "fp32", "ngf": 64, "batch": 32,
                     "chunk": 32, "sigma": 4.0, "rows": rows, "last_smoothed_run": clip_facts}
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
