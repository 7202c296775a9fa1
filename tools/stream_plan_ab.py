#!/usr/bin/env python3
"""Identity A/B of the streaming stabiliser across a refactor: run the same small clips through VideoStabilizer.run_video / run with two builds
of the package and compare, per case, the SHA-256 of the output, of every result attribute that is a tensor (repr for lists and floats) and
the ordered list of C entries called (hipabi.check is wrapped: every launch passes its entry's name there; no kernel runs twice for this).

One build per process, each under its own time limit; the second checkout holds the other commit, built:

    timeout -k 10 600 python tools/stream_plan_ab.py --root ../parent --json profiles/stream_plan_ab_parent.json && \\
    timeout -k 10 600 python tools/stream_plan_ab.py --json profiles/stream_plan_ab_head.json && \\
    python tools/stream_plan_ab.py --compare profiles/stream_plan_ab_parent.json profiles/stream_plan_ab_head.json

Clips: 40 frames of 600 x 300 (the smallest size with the homography lattice and W % 4 == 0), chunk 16, batch 8, the tests' small generator
(ngf 16, synth weights, seed 123), a hard cut at frame 21 where cuts are used.  --compare exits 1 on any difference, naming the case and key."""
import argparse
import hashlib
import json
import os
import sys

T, H, W, CUT = 40, 300, 600, 21
RESULTS = ("zoom_windows", "zoom_uncovered", "rigid_residual", "rigid_unfit", "mosaic_unfilled", "motion_in", "motion_out", "motion_inliers_in",
           "motion_inliers_out", "_report", "smooth_motion", "smooth_inliers", "smooth_path", "smooth_correction", "smooth_uncovered",
           "shutter_rates", "shutter_estimate", "rolling_shutter_used", "limit_strength", "limit_need", "limit_uncovered",
           "smooth_correction_unlimited", "wobble_removed", "wobble_unfit", "scene_cuts")

# name -> (constructor kwargs, pixel format, frames on the host, run_video kwargs)
CASES = {
    "a_bgr24_host_half": ({}, "bgr24", True, {"half_size_output": True}),
    "b_bgr24_device_half_in_flight2": ({}, "bgr24", False, {"half_size_output": True, "in_flight": 2}),
    "c_nv12_output_size_crop_cuts": ({}, "nv12", True, {"output_size": (300, 150), "crop": (4, 296, 2, 148), "scene_cuts": [CUT]}),
    "d_p010_cuts_auto": ({}, "p010", True, {"scene_cuts": "auto"}),
    "e_keep_in_flight2_cuts": ({"borders": "keep"}, "bgr24", False, {"in_flight": 2, "scene_cuts": [CUT]}),
    "f_mosaic4_mirror_cuts_halos": ({"borders": "mosaic", "mosaic_radius": 4, "edge": "mirror"}, "bgr24", True,
                                    {"scene_cuts": [CUT], "halo_left": 3, "halo_right": 2}),
    "g_rigid_zoom_metrics": ({"rigidity": 0.5}, "bgr24", False, {"zoom": 0.9, "metrics": True}),
    "h_crop_auto_rigid1": ({"rigidity": 1.0}, "bgr24", True, {"crop": "auto"}),
    "i_zoom_auto_i422_clamp": ({"edge": "clamp"}, "i422", False, {"zoom": "auto"}),
    "j_zoom_adaptive_bicubic": ({"interpolation": "bicubic"}, "bgr24", False, {"zoom": "adaptive"}),
    "k_smooth_crop_auto_metrics": ({"smooth": 2.0}, "bgr24", True, {"crop": "auto", "metrics": True}),
    "l_smooth_shutter_limit_zoom": ({"smooth": 2.0, "rolling_shutter": 0.3, "max_crop": 0.1}, "bgr24", False, {"zoom": 0.9}),
    "m_smooth_shutter_auto_wobble": ({"smooth": 2.0, "rolling_shutter": "auto", "wobble": 1.0}, "bgr24", False, {"scene_cuts": [CUT]}),
    "n_wobble_i410": ({"wobble": 1.0}, "i410", False, {}),
    "o_halos15_in_flight2": ({}, "bgr24", True, {"halo_left": 15, "halo_right": 15, "in_flight": 2}),
    "p_no_frame": ({}, "bgr24", True, {"frames": 0}),
    "p_one_frame": ({}, "bgr24", True, {"frames": 1}),
}


def digest(v):
    import torch
    if isinstance(v, torch.Tensor):
        t = v.detach().to("cpu").contiguous().reshape(-1)
        return "sha256:%s:%s:%s" % (str(t.dtype)[6:], "x".join(map(str, t.shape)), hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest())
    if isinstance(v, dict):
        return {k: digest(x) for k, x in sorted(v.items())}
    return repr(v)


def clip(pixel_format, n=T):
    """Two smooth scenes under small per-frame translations (synth.smooth_frames_u8), cut at CUT, as frames of the format."""
    import numpy as np
    import torch
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import synth
    base = np.concatenate([synth.smooth_frames_u8(1, CUT, H, W, 17)[0], synth.smooth_frames_u8(1, T - CUT, H, W, 18)[0]])[:n]
    rs = np.random.RandomState(17)
    fmt = PF.lookup_format(pixel_format)
    if not fmt.packed:
        col = np.stack([base * 0.9, base * 1.0, base * 0.8], -1) + rs.randint(-3, 4, (n, H, W, 3))
        return torch.from_numpy(np.clip(col, 0, 255).astype(np.uint8))
    out = rs.randint(96, 160, (n, fmt.packed_rows(H), W)).astype(np.int64)   # (the chroma rows)
    out[:, :H] = 16 + base.astype(np.int64) * 219 // 255
    if fmt.dtype == torch.uint16:   # 10 bits: in the low bits of a word for the planar layouts, in the high bits for P010 / P210
        out = out * 4 << (6 if fmt.layout == 0 else 0)
        return torch.from_numpy(out.astype(np.uint16))
    return torch.from_numpy(out.astype(np.uint8))


def record(vs, fn):
    """fn()'s output and what it left on ``vs``, with the C entries it called in their order."""
    import torch
    from pwstablenet_amd import hipabi
    calls, real = [], hipabi.check

    def check(rc, what=""):
        calls.append(what)
        return real(rc, what)
    hipabi.check = check
    try:
        res = {"out": digest(fn())}   # (every case is meant to run: an exception ends the tool)
        torch.cuda.synchronize()
    finally:
        hipabi.check = real
    res["results"] = {k: digest(getattr(vs, k)) for k in RESULTS if getattr(vs, k) is not None}   # (an attribute that is not listed is None)
    res["entries"] = calls
    return res


def run_cases():
    import torch
    from pwstablenet_amd import synth
    from pwstablenet_amd.lib.networks_cascading import define_G
    from pwstablenet_amd.stream import VideoStabilizer, window_planes
    torch.manual_seed(0)
    net = define_G(31, 2, 16, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=16)})
    net = net.cuda()
    out = {}
    for name, (ctor, fmt, host, kw) in CASES.items():
        kw = dict(kw)
        frames = clip(fmt, kw.pop("frames", T))
        frames = frames.pin_memory() if host else frames.cuda()
        vs = VideoStabilizer(net, batch=8, swap_rb=True, **ctor)
        out[name] = record(vs, lambda: vs.run_video(frames, chunk=16, pixel_format=fmt, **kw))
        print(name, out[name]["out"], len(out[name]["entries"]), "entries", flush=True)
    # q: run() alone
    bgr = clip("bgr24").cuda()
    gray = window_planes(bgr)
    vs = VideoStabilizer(net, batch=8)
    floats = bgr.permute(0, 3, 1, 2).float().contiguous()
    out["q_run_device_float"] = record(vs, lambda: vs.run(gray, floats))
    vs = VideoStabilizer(net, batch=8, swap_rb=True)
    host = bgr.cpu().pin_memory()
    out["q_run_host_u8_zoom"] = record(vs, lambda: vs.run(gray.cpu(), host, zoom=(30.0, 570.0, 15.0, 285.0), scene_cuts=[CUT]))
    for name in ("q_run_device_float", "q_run_host_u8_zoom"):
        print(name, out[name]["out"], len(out[name]["entries"]), "entries", flush=True)
    return out


def compare(a, b):
    with open(a) as f:
        x = json.load(f)["cases"]
    with open(b) as f:
        y = json.load(f)["cases"]
    bad = []
    for name in sorted(set(x) | set(y)):
        if name not in x or name not in y:
            bad.append("%s: in one file only" % name)
            continue
        for key in sorted(set(x[name]) | set(y[name])):
            if x[name].get(key) != y[name].get(key):
                bad.append("%s: %s differs" % (name, key))
    print("\n".join(bad) if bad else "identical: %d cases, outputs, result attributes and entry lists" % len(x))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package runs")
    ap.add_argument("--json")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    sys.path.insert(0, os.path.abspath(args.root))
    import pwstablenet_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(pwstablenet_amd.__file__))) == os.path.abspath(args.root), pwstablenet_amd.__file__
    write(args.json, run_cases())


def write(path, cases):
    with open(path, "w") as f:   # (a case a line)
        f.write('{"frames": %s, "cases": {\n%s\n}}\n' % (json.dumps([T, H, W]), ",\n".join(
            "%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(cases.items()))))


if __name__ == "__main__":
    main()
